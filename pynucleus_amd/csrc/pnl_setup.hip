// libpnl_hip.so -- the host-only part of the C ABI of include/pnl_hip.h: nothing here is or launches a kernel.
//
// Context lifecycle and options, every upload and setter, finalize() (the tables derived from mesh + DoF map: padded SoA cell
// arrays, unique DoFs per block, touching cell and cell/facet pairs, block-slot storage), the vertex-order search of the tile
// kernels, the power tables and the problem description of a class (pnl_refresh_tables), the tile plan (pnl_make_tiles,
// pnl_upload_tiles: which tiles are of one order, the tile lists per class / of the single-launch P2 layout), the state of the
// orders per quadrature point, counters and timers.  The one kernel the tile plan needs, k_tile_order_range, is launched by
// pnl_tile_order_range (pnl_hip.hip); what the launching units need from here is declared in pnl_context.h.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "pnl_hip.h"
#include "pnl_context.h"

// body(th, nthr) on up to eight host threads th = 0 .. nthr-1, joined before the return; the caller splits its index range
template <class F>
static void host_threads(F body, int want = 0) {
    const int nthr = want > 0 ? std::min(want, 64) : (int)std::max(1u, std::min(8u, std::thread::hardware_concurrency()));
    std::vector<std::thread> pool;
    for (int th = 0; th < nthr; th++) pool.emplace_back([&body, th, nthr]() { body(th, nthr); });
    for (auto &t : pool) t.join();
}

// vertex order of the cells for the tile kernels (see finalize): search on host threads, tables on first use
struct TileOrderJob {
    std::vector<int> cells, lperm;
    int nc = 0, T = 0, nblocks = 0, ncp = 0, dim = 0, dpe = 0;
    std::vector<double> cellv;
    std::vector<int32_t> cdof;
    std::vector<int16_t> cslot;
    int nU = 0;
    UniLaneTables lanes[3];
    double lanes_seconds = 0.;
    std::thread worker;
};

static void tile_order_drop(pnl_context *ctx) {
    if (!ctx->tile_job) return;
    if (ctx->tile_job->worker.joinable()) ctx->tile_job->worker.join();
    delete ctx->tile_job;
    ctx->tile_job = nullptr;
}

// the launching units (pnl_hip.hip, pnl_slab.hip): the Dt half of the per-cell diagonal blocks exists iff the permuted tables do; a context
// that was finalized again since the assembly (setKernel, pnl_set_cell_order) holds the flag false until the job is joined
int pnl_tile_order_ready(pnl_context *ctx) {
    TileOrderJob *job = ctx->tile_job;
    if (!job) return PNL_OK;
    if (job->worker.joinable()) job->worker.join();
    for (int m = 0; m < 3; m++) ctx->uni_lanes[m] = std::move(job->lanes[m]);
    ctx->uni_lanes_seconds = job->lanes_seconds;
    ctx->uni_lanes_up = -1;
    const int nV = job->dim+1, NC = nV*job->dim, ncp = job->ncp, dpe = job->dpe, dim = job->dim;
    std::vector<double> cellv_t((size_t)NC*ncp, 0.);
    std::vector<int32_t> cdof_t((size_t)dpe*ncp, -1);
    std::vector<int16_t> cslot_t((size_t)dpe*ncp, -1);
    for (int c = 0; c < job->nc; c++)
        for (int k = 0; k < nV; k++) {
            const int src = job->lperm[(size_t)c*nV+k];
            for (int d = 0; d < dim; d++) cellv_t[(size_t)(k*dim+d)*ncp+c] = job->cellv[(size_t)(src*dim+d)*ncp+c];
            cdof_t[(size_t)k*ncp+c] = job->cdof[(size_t)src*ncp+c];
            cslot_t[(size_t)k*ncp+c] = job->cslot[(size_t)src*ncp+c];
        }
    int rc2;
    ctx->ul_cellv_t = cellv_t;
    ctx->ul_cslot_t.assign(cslot_t.begin(), cslot_t.end());
    if ((rc2 = upload(ctx, ctx->b_cellv_t, cellv_t.data(), cellv_t.size()))) return rc2;
    if ((rc2 = upload(ctx, ctx->b_cdof_t, cdof_t.data(), cdof_t.size()))) return rc2;
    if ((rc2 = upload(ctx, ctx->b_cslot_t, cslot_t.data(), cslot_t.size()))) return rc2;
    if ((rc2 = ensure(ctx, ctx->b_Dt, sizeof(double)*(size_t)ncp*(dpe*(dpe+1)/2)))) return rc2;
    ctx->have_tile_order = true;
    delete job;
    ctx->tile_job = nullptr;
    return PNL_OK;
}

// P1: for DISTANT pairs the local vertex order of a cell is free (symmetric rules; touching pairs keep the reference's
// order, their rules are not invariant).  The tile kernels read a copy of the cell tables in which the order is chosen
// per cell so that within a block of T cells a vertex appears at every local position about equally often: the lanes of
// a ds_add_f64 then hit the same LDS address ~2.3 instead of ~4.3 times (greedy + local search).
// The search runs on host threads of its own (0.24 s on one thread at 98,304 cells, 30-50 ms on eight) and is waited for by the
// first dense assembly (pnl_tile_order_ready): the near-field / H2 path never reads the permuted tables, and a dense assembly
// overlaps it with the rest of finalize() and with the uploads of rules and kernels.
static void tile_order_block(int b, int nc, int T, const int *cells, int *lperm) {
    static const int perms[6][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}, {0, 2, 1}, {2, 1, 0}, {1, 0, 2}};
    std::vector<std::pair<long long, int>> seen;   // (vertex*3+pos) -> count, small per block
    auto get = [&](int v, int pos) { for (auto &e : seen) if (e.first == (long long)v*3+pos) return e.second; return 0; };
    auto add = [&](int v, int pos, int d) { for (auto &e : seen) if (e.first == (long long)v*3+pos) { e.second += d; return; } seen.push_back({(long long)v*3+pos, d}); };
    // greedy pass, then a few sweeps of local search (every cell re-chooses its order given all the others)
    for (int sweep = 0; sweep < 5; sweep++)
        for (int c = b*T; c < std::min(nc, (b+1)*T); c++) {
            if (sweep) for (int k = 0; k < 3; k++) add(cells[(size_t)c*3+lperm[(size_t)c*3+k]], k, -1);
            int best = 0, bestmax = 1 << 30, bestsum = 1 << 30;
            for (int p = 0; p < 6; p++) {
                int mx = 0, sum = 0;
                for (int k = 0; k < 3; k++) { const int g = get(cells[(size_t)c*3+perms[p][k]], k); mx = std::max(mx, g); sum += g*g; }
                if (mx < bestmax || (mx == bestmax && sum < bestsum)) { best = p; bestmax = mx; bestsum = sum; }
            }
            for (int k = 0; k < 3; k++) { lperm[(size_t)c*3+k] = perms[best][k]; add(cells[(size_t)c*3+perms[best][k]], k, 1); }
        }
}

// ---- lane layout of a block for k_tile_uniform (2D P1) ------------------------------------------------------------------------
// ds_add_f64 serves a wave in four groups of 16 contiguous lanes, 16 double-banks (tools/probes/lds_atomic_probe.hip: distinct banks
// inside every group 8.1 cycles whatever the other groups do, n lanes of a group on one bank n times that, the cost is the sum over the
// groups; two lanes on one ADDRESS 2.5 times).  In k_tile_uniform the lanes own the cells of the column block and the row stride of the
// sub-block is a multiple of 16 doubles, so the bank of the add (local position k of the lane's cell, any row) is the column of that
// DoF mod 16: the same for every step of the rotation and every partner block.  Free per block: which cell sits in which lane, and the
// column of every DoF.  The vertex order of the cells is the one of the order search above (shared with the mixed-tile kernels, whose
// tables therefore do not change).  Objective: over the 12 classes (lane group, local position), the pairs of lanes on one residue.
// Min-conflicts search: a lane of a loaded residue either trades places with a lane of another group or its DoF takes another
// residue (at most cap DoFs per residue, trading with one of that residue's DoFs when it is full); the best move is taken if it does
// not raise the objective.  Seeded per block, so the result does not depend on the number of host threads.
// mode 0: identity (lane = cell, column = slot, trash column nUe); 1: searched; 2: random lanes and columns (tests: a bad layout)
namespace {
struct LaneSearch {
    int cnt[4][3][16], cost = 0;
    int dof[64][3];                               // slot of (cell of the block, local position), -1: none
    int lane_of[64], cell_at[64];
    std::vector<int> res, inc_off, inc;           // residue per slot; incidences (cell << 2 | position) per slot
    int nres[16];
    unsigned long long rng;
    unsigned next() { rng ^= rng << 13; rng ^= rng >> 7; rng ^= rng << 17; return (unsigned)(rng >> 11); }
    void bump(int g, int k, int r, int s) { int &c = cnt[g][k][r]; if (s > 0) { cost += c; c++; } else { c--; cost -= c; } }
    void cell(int c, int g, int s) { for (int k = 0; k < 3; k++) if (dof[c][k] >= 0) bump(g, k, res[dof[c][k]], s); }
    void swap_lanes(int p, int q) {
        const int cp = cell_at[p], cq = cell_at[q], gp = p >> 4, gq = q >> 4;
        if (gp != gq) { cell(cp, gp, -1); cell(cq, gq, -1); cell(cp, gq, 1); cell(cq, gp, 1); }
        cell_at[p] = cq; cell_at[q] = cp; lane_of[cp] = q; lane_of[cq] = p;
    }
    void set_res(int d, int r) {
        for (int e = inc_off[d]; e < inc_off[d+1]; e++) {
            const int g = lane_of[inc[e] >> 2] >> 4, k = inc[e] & 3;
            bump(g, k, res[d], -1); bump(g, k, r, 1);
        }
        nres[res[d]]--; nres[r]++; res[d] = r;
    }
    double multiplier() const {
        double m = 0.;
        for (int g = 0; g < 4; g++) for (int k = 0; k < 3; k++) { int mx = 1; for (int r = 0; r < 16; r++) mx = std::max(mx, cnt[g][k][r]); m += mx; }
        return m/12.;
    }
};
}  // namespace

// columns of the searched / random layouts: cap = ceil(nU / 16) DoFs per residue, then 16 trash columns
static int uni_lane_cap(int nU) { return std::max(1, (nU+15)/16); }

static void uni_lane_block(int b, int ncp, int nU, const int16_t *cslot_t, int mode, UniLaneTables &out) {
    const int nUe = (nU+1) & ~1, cap = uni_lane_cap(nU), ncol = 16*cap;
    unsigned char *lane_cell = out.lane_cell.data()+(size_t)b*64;
    short *lds_col = out.lds_col.data()+(size_t)b*nU;
    LaneSearch S;
    std::memset(S.cnt, 0, sizeof(S.cnt)); std::memset(S.nres, 0, sizeof(S.nres));
    S.rng = 0x9E3779B97F4A7C15ull*(unsigned long long)(b+1)+(unsigned long long)mode;
    for (int c = 0; c < 64; c++) for (int k = 0; k < 3; k++) S.dof[c][k] = cslot_t[(size_t)k*ncp+b*64+c];
    S.res.assign(nU, 0); S.inc_off.assign(nU+1, 0);
    for (int c = 0; c < 64; c++) for (int k = 0; k < 3; k++) if (S.dof[c][k] >= 0) S.inc_off[S.dof[c][k]+1]++;
    for (int d = 0; d < nU; d++) S.inc_off[d+1] += S.inc_off[d];
    S.inc.assign(S.inc_off[nU], 0);
    { std::vector<int> fill(S.inc_off.begin(), S.inc_off.end()-1);
      for (int c = 0; c < 64; c++) for (int k = 0; k < 3; k++) if (S.dof[c][k] >= 0) S.inc[fill[S.dof[c][k]]++] = c << 2 | k; }
    for (int l = 0; l < 64; l++) S.lane_of[l] = S.cell_at[l] = l;
    if (mode == 0) {
        for (int l = 0; l < 64; l++) lane_cell[l] = (unsigned char)l;
        for (int d = 0; d < nU; d++) lds_col[d] = (short)d;
        for (int c = 0; c < 64; c++) for (int k = 0; k < 3; k++) out.cell_col[(size_t)k*ncp+b*64+c] = (short)(S.dof[c][k] >= 0 ? S.dof[c][k] : nUe);
        out.mult[b] = 0.;                             // depends on the partner block (bank = row + column): see the tests
        return;
    }
    if (mode == 2) {
        for (int l = 63; l > 0; l--) { const int m = (int)(S.next()%(unsigned)(l+1)); std::swap(S.cell_at[l], S.cell_at[m]); }
        for (int l = 0; l < 64; l++) S.lane_of[S.cell_at[l]] = l;
        std::vector<int> cols(ncol);
        for (int i = 0; i < ncol; i++) cols[i] = i;
        for (int i = ncol-1; i > 0; i--) std::swap(cols[i], cols[S.next()%(unsigned)(i+1)]);
        for (int d = 0; d < nU; d++) { lds_col[d] = (short)cols[d]; S.res[d] = cols[d] & 15; }
        for (int c = 0; c < 64; c++) S.cell(c, S.lane_of[c] >> 4, 1);
        for (int c = 0; c < 64; c++) for (int k = 0; k < 3; k++) {
            const int t = ncol+(int)(S.next() & 15);
            if (S.dof[c][k] < 0) S.bump(S.lane_of[c] >> 4, k, t & 15, 1);
            out.cell_col[(size_t)k*ncp+b*64+c] = (short)(S.dof[c][k] >= 0 ? lds_col[S.dof[c][k]] : t);
        }
        for (int l = 0; l < 64; l++) lane_cell[l] = (unsigned char)S.cell_at[l];
        out.mult[b] = S.multiplier();
        return;
    }
    // searched: start from residue = slot mod 16 (at most cap per residue), lanes in cell order
    for (int d = 0; d < nU; d++) { S.res[d] = d & 15; S.nres[d & 15]++; }
    for (int c = 0; c < 64; c++) S.cell(c, c >> 4, 1);
    std::vector<int> best_res = S.res;
    int best_cell_at[64], best_cost = S.cost;
    std::memcpy(best_cell_at, S.cell_at, sizeof(best_cell_at));
    const int max_steps = 600;
    for (int step = 0; step < max_steps && best_cost > 0; step++) {
        // a lane and position on a loaded residue, from a random start
        int p = -1, k = 0;
        const unsigned start = S.next()%192u;
        for (unsigned t = 0; t < 192u; t++) {
            const unsigned e = (start+t)%192u;
            const int l = (int)(e/3u), kk = (int)(e%3u), d = S.dof[S.cell_at[l]][kk];
            if (d >= 0 && S.cnt[l >> 4][kk][S.res[d]] > 1) { p = l; k = kk; break; }
        }
        if (p < 0) break;
        const int d = S.dof[S.cell_at[p]][k], c0 = S.cost;
        // candidates: kind 0 trade lanes p, q; kind 1 residue r for d (trading with DoF e if r is full)
        int bk = -1, bx = 0, by = -1, bcost = 1 << 30, nties = 0;
        auto consider = [&](int kind, int x, int y) {
            if (S.cost < bcost) { bcost = S.cost; nties = 0; }
            if (S.cost == bcost && S.next()%(unsigned)(++nties) == 0) { bk = kind; bx = x; by = y; }
        };
        for (int q = 0; q < 64; q++) {
            if ((q >> 4) == (p >> 4)) continue;
            S.swap_lanes(p, q); consider(0, q, -1); S.swap_lanes(p, q);
        }
        const int r0 = S.res[d];
        for (int r = 0; r < 16; r++) {
            if (r == r0) continue;
            if (S.nres[r] < cap) { S.set_res(d, r); consider(1, r, -1); S.set_res(d, r0); }
            else
                for (int e = 0; e < nU; e++) {
                    if (S.res[e] != r) continue;
                    S.set_res(e, r0); S.set_res(d, r); consider(1, r, e); S.set_res(d, r0); S.set_res(e, r);
                }
        }
        if (bk < 0 || bcost > c0) continue;               // no move that does not raise the objective: another lane next time
        if (bk == 0) S.swap_lanes(p, bx);
        else { if (by >= 0) S.set_res(by, r0); S.set_res(d, bx); }
        if (S.cost < best_cost) { best_cost = S.cost; best_res = S.res; std::memcpy(best_cell_at, S.cell_at, sizeof(best_cell_at)); }
    }
    // the best state, counted again; trash columns: per class the lanes without a DoF take residues no lane of the class holds
    std::memset(S.cnt, 0, sizeof(S.cnt)); S.cost = 0;
    S.res = best_res;
    for (int l = 0; l < 64; l++) { S.cell_at[l] = best_cell_at[l]; S.lane_of[best_cell_at[l]] = l; }
    for (int c = 0; c < 64; c++) S.cell(c, S.lane_of[c] >> 4, 1);
    { int used[16] = {};
      for (int d = 0; d < nU; d++) lds_col[d] = (short)(S.res[d]+16*used[S.res[d]]++); }
    for (int g = 0; g < 4; g++)
        for (int k = 0; k < 3; k++) {
            int r = 0;
            for (int l = 16*g; l < 16*g+16; l++) {
                const int c = S.cell_at[l], d = S.dof[c][k];
                short col;
                if (d >= 0) col = lds_col[d];
                else {
                    while (r < 16 && S.cnt[g][k][r] > 0) r++;
                    const int rr = r < 16 ? r : 0;
                    S.bump(g, k, rr, 1);
                    col = (short)(ncol+rr);
                }
                out.cell_col[(size_t)k*ncp+b*64+c] = col;
            }
        }
    for (int l = 0; l < 64; l++) lane_cell[l] = (unsigned char)S.cell_at[l];
    out.mult[b] = S.multiplier();
}

// the tables of all three settings of PNL_UNI_LANES for every block; cslot_t: [3][ncp] slots in the tile kernels' vertex order
static void uni_lane_layout(int nblocks, int ncp, int nU, const int16_t *cslot_t, UniLaneTables (&out)[3], int nthreads = 0) {
    for (int m = 0; m < 3; m++) {
        out[m].lane_cell.assign((size_t)nblocks*64, 0); out[m].lds_col.assign((size_t)nblocks*nU, 0);
        out[m].cell_col.assign((size_t)3*ncp, 0); out[m].mult.assign(nblocks, 0.);
        out[m].stride = m == 0 ? 0 : 16*uni_lane_cap(nU)+16;
    }
    host_threads([&](int th, int nthr) {
        for (int b = th; b < nblocks; b += nthr)
            for (int m = 0; m < 3; m++) uni_lane_block(b, ncp, nU, cslot_t, m, out[m]);
    }, nthreads);
}

static void tile_order_search(TileOrderJob *job) {
    const int nc = job->nc, T = job->T, nblocks = job->nblocks, ncp = job->ncp;
    // the blocks are independent: a few host threads
    host_threads([&](int th, int nthr) {
        for (int b = th; b < nblocks; b += nthr) tile_order_block(b, nc, T, job->cells.data(), job->lperm.data());
    });
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int16_t> cslot_t((size_t)3*ncp, -1);
    for (int c = 0; c < nc; c++) for (int k = 0; k < 3; k++) cslot_t[(size_t)k*ncp+c] = job->cslot[(size_t)job->lperm[(size_t)c*3+k]*ncp+c];
    uni_lane_layout(nblocks, ncp, job->nU, cslot_t.data(), job->lanes);
    job->lanes_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now()-t0).count();
}

// the lane layout of the option in force on the device (uploaded when the option or the tables changed)
int pnl_uni_lanes_ready(pnl_context *ctx, UniLanes *UL, int *mode, int *stride) {
    int rc = pnl_tile_order_ready(ctx);
    if (rc) return rc;
    int m = pnl_tune("PNL_UNI_LANES") ? atoi(pnl_tune("PNL_UNI_LANES")) : 1;
    if (m < 0 || m > 2) return fail(ctx, PNL_ERR_INVALID, "PNL_UNI_LANES = %d (0 identity, 1 searched, 2 random)", m);
    const UniLaneTables &T = ctx->uni_lanes[m];
    if (T.lane_cell.empty()) return fail(ctx, PNL_ERR_STATE, "no lane layout (2D P1 only)");
    if (ctx->uni_lanes_up != m) {
        if ((rc = upload(ctx, ctx->b_ul_cell, T.lane_cell.data(), T.lane_cell.size()))) return rc;
        if ((rc = upload(ctx, ctx->b_ul_col, T.lds_col.data(), T.lds_col.size()))) return rc;
        // the cell tables in lane order
        const int ncp = ctx->ncp, nc = ctx->nc;
        std::vector<double> cellv((size_t)6*ncp), cvol(ncp);
        std::vector<short> cslot((size_t)3*ncp), ccol((size_t)3*ncp);
        std::vector<unsigned char> real(ncp);
        for (int p = 0; p < ncp; p++) {
            const int c = (p & ~63)+T.lane_cell[p];
            for (int k = 0; k < 6; k++) cellv[(size_t)k*ncp+p] = ctx->ul_cellv_t[(size_t)k*ncp+c];
            for (int k = 0; k < 3; k++) { cslot[(size_t)k*ncp+p] = ctx->ul_cslot_t[(size_t)k*ncp+c]; ccol[(size_t)k*ncp+p] = T.cell_col[(size_t)k*ncp+c]; }
            cvol[p] = c < nc ? ctx->vol[c] : 0.;
            real[p] = c < nc && ctx->vol[c] != 0.;
        }
        if ((rc = upload(ctx, ctx->b_ul_ccol, ccol.data(), ccol.size()))) return rc;
        if ((rc = upload(ctx, ctx->b_ul_cellv, cellv.data(), cellv.size()))) return rc;
        if ((rc = upload(ctx, ctx->b_ul_cvol, cvol.data(), cvol.size()))) return rc;
        if ((rc = upload(ctx, ctx->b_ul_cslot, cslot.data(), cslot.size()))) return rc;
        if ((rc = upload(ctx, ctx->b_ul_real, real.data(), real.size()))) return rc;
        ctx->uni_lanes_up = m;
    }
    UL->lane_cell = (const unsigned char*)ctx->b_ul_cell.p; UL->lds_col = (const short*)ctx->b_ul_col.p; UL->cell_col = (const short*)ctx->b_ul_ccol.p;
    UL->cellv = (const double*)ctx->b_ul_cellv.p; UL->cvol = (const double*)ctx->b_ul_cvol.p; UL->cslot = (const short*)ctx->b_ul_cslot.p;
    UL->real = (const unsigned char*)ctx->b_ul_real.p;
    *mode = m; *stride = T.stride;
    return PNL_OK;
}

// ---- finalize(): everything derived from mesh + DoF map, in steps ---------------------------------------------------------
// the host tables the steps hand to each other
struct CellTables {
    int dim, nV, nc, dpe, T, nblocks, ncp;
    std::vector<double> cellv, ccen, cvol, ch;
    std::vector<int32_t> cvid, cdof;
    std::vector<char> dummy;                  // cell of volume zero
    std::vector<std::vector<int>> lists;      // unique DoFs per block
    std::vector<int32_t> blk_ndof, blk_dofs;
    std::vector<int16_t> cslot;
    std::vector<int> vptr, vcells;            // vertex -> cells adjacency (real cells)
};

static void start_tile_order_search(pnl_context *ctx, const CellTables &F) {
    const int nc = F.nc, nV = F.nV;
    TileOrderJob *job = new TileOrderJob;
    ctx->tile_job = job;
    job->cells = ctx->cells;
    job->nc = nc; job->T = F.T; job->nblocks = F.nblocks; job->ncp = F.ncp; job->dim = F.dim; job->dpe = F.dpe;
    job->nU = ctx->nU;
    job->cellv = F.cellv; job->cdof = F.cdof; job->cslot = F.cslot;   // the lane layout reads the slots: before the worker starts
    job->lperm.resize((size_t)nc*nV);
    for (int c = 0; c < nc; c++) for (int k = 0; k < nV; k++) job->lperm[(size_t)c*nV+k] = k;
    job->worker = std::thread(tile_order_search, job);
}

// Cells of volume ZERO are padding inside the mesh (builder.label_blocks: a block of cells that would straddle an interface
// of a piecewise-constant order is split into one block per label, filled up with zero-volume copies of its own cells).
// They keep their geometry (every kernel value stays finite), carry no DoFs, negative vertex ids like the padding behind
// the last cell (the tile kernels drop every pair that holds one), and belong to no touching pair.
static int padded_cell_tables(pnl_context *ctx, CellTables &F) {
    const int dim = F.dim, nV = F.nV, nc = F.nc, dpe = F.dpe, ncp = F.ncp;
    std::vector<double> &cellv = F.cellv, &ccen = F.ccen, &cvol = F.cvol, &ch = F.ch;
    std::vector<int32_t> &cvid = F.cvid, &cdof = F.cdof;
    std::vector<char> &dummy = F.dummy;
    cellv.assign((size_t)nV*dim*ncp, 0.); ccen.assign((size_t)dim*ncp, 0.); cvol.assign(ncp, 0.); ch.assign(ncp, 1.);
    cvid.resize((size_t)nV*ncp); cdof.assign((size_t)dpe*ncp, -1);
    ctx->nreal = 0;
    dummy.assign(nc, 0);
    for (int c = 0; c < nc; c++) { dummy[c] = ctx->vol[c] == 0.; ctx->nreal += !dummy[c]; }
    ctx->real_from.assign((size_t)nc+1, 0);                  // number of real cells with index >= c
    for (int c = nc-1; c >= 0; c--) ctx->real_from[c] = ctx->real_from[c+1]+(dummy[c] ? 0 : 1);
    for (int c = 0; c < ncp; c++) {
        for (int k = 0; k < nV; k++) cvid[(size_t)k*ncp+c] = -1-k;
        if (c >= nc) continue;
        double cen[2] = {0., 0.};
        for (int k = 0; k < nV; k++) {
            const int v = ctx->cells[(size_t)c*nV+k];
            if (v < 0 || v >= ctx->nv) return fail(ctx, PNL_ERR_INVALID, "cell %d references vertex %d", c, v);
            if (!dummy[c]) cvid[(size_t)k*ncp+c] = v;
            for (int d = 0; d < dim; d++) {
                const double x = ctx->vertices[(size_t)v*dim+d];
                // the quadrature points and the cut-element geometry live in the coordinates of the interaction transform (all
                // they enter is differences x - y: |T (x - y)|, interactionDomains.pyx:1417-1470); centres, h and volumes -- the order
                // formula and the measure -- stay those of the mesh
                double xt = x;
                if (ctx->have_xform && dim == 2) xt = ctx->xform[2*d]*ctx->vertices[(size_t)v*dim]+ctx->xform[2*d+1]*ctx->vertices[(size_t)v*dim+1];
                cellv[(size_t)(k*dim+d)*ncp+c] = xt;
                cen[d] += x;
            }
        }
        const double fac = 1./nV;                    // NO:116-126
        for (int d = 0; d < dim; d++) ccen[(size_t)d*ncp+c] = cen[d]*fac;
        cvol[c] = ctx->vol[c];
        ch[c] = ctx->h[c];
        for (int k = 0; k < dpe; k++) {
            const int g = ctx->dofs[(size_t)c*dpe+k];
            if (g >= ctx->N) return fail(ctx, PNL_ERR_INVALID, "DoF id %d >= num_dofs %d", g, ctx->N);
            if (dummy[c] && g >= 0) return fail(ctx, PNL_ERR_INVALID, "cell %d has volume zero and a DoF", c);
            cdof[(size_t)k*ncp+c] = g;
        }
    }
    return PNL_OK;
}

// unique DoFs per block
static void block_dofs(pnl_context *ctx, CellTables &F) {
    const int nc = F.nc, dpe = F.dpe, T = F.T, nblocks = F.nblocks, ncp = F.ncp;
    std::vector<std::vector<int>> &lists = F.lists;
    std::vector<int32_t> &blk_ndof = F.blk_ndof, &blk_dofs = F.blk_dofs, &cdof = F.cdof;
    std::vector<int16_t> &cslot = F.cslot;
    lists.assign(nblocks, std::vector<int>());
    int nU = 1;
    for (int b = 0; b < nblocks; b++) {
        auto &L = lists[b];
        for (int c = b*T; c < std::min(nc, (b+1)*T); c++)
            for (int k = 0; k < dpe; k++) {
                const int g = ctx->dofs[(size_t)c*dpe+k];
                if (g >= 0) L.push_back(g);
            }
        std::sort(L.begin(), L.end());
        L.erase(std::unique(L.begin(), L.end()), L.end());
        nU = std::max<int>(nU, (int)L.size());
    }
    ctx->nU = nU;
    blk_ndof.assign(nblocks, 0); blk_dofs.assign((size_t)nblocks*nU, 0);
    cslot.assign((size_t)dpe*ncp, -1);
    for (int b = 0; b < nblocks; b++) {
        auto &L = lists[b];
        blk_ndof[b] = (int)L.size();
        std::copy(L.begin(), L.end(), blk_dofs.begin()+(size_t)b*nU);
        for (int c = b*T; c < std::min(nc, (b+1)*T); c++)
            for (int k = 0; k < dpe; k++) {
                const int g = cdof[(size_t)k*ncp+c];
                if (g >= 0) cslot[(size_t)k*ncp+c] = (int16_t)(std::lower_bound(L.begin(), L.end(), g)-L.begin());
            }
    }
}

// touching cell pairs via vertex -> cells adjacency (NO:311-323 shared-vertex test, done once)
static int touching_cell_pairs(pnl_context *ctx, CellTables &F) {
    const int nV = F.nV, nc = F.nc;
    const std::vector<char> &dummy = F.dummy;
    std::vector<int> &vptr = F.vptr, &vcells = F.vcells;
    vptr.assign(ctx->nv+1, 0);
    for (int c = 0; c < nc; c++)
        for (int k = 0; k < nV && !dummy[c]; k++) vptr[ctx->cells[(size_t)c*nV+k]+1]++;
    for (int v = 0; v < ctx->nv; v++) vptr[v+1] += vptr[v];
    vcells.assign(vptr[ctx->nv], 0);
    std::vector<int> fill(vptr.begin(), vptr.end()-1);
    for (int c = 0; c < nc; c++)
        for (int k = 0; k < nV && !dummy[c]; k++) vcells[fill[ctx->cells[(size_t)c*nV+k]]++] = c;
    for (int s = 0; s < 3; s++) ctx->spairs_host[s].clear();
    {
        std::vector<int> nbr;
        for (int c1 = 0; c1 < nc; c1++) {
            nbr.clear();
            if (dummy[c1]) continue;
            for (int k = 0; k < nV; k++) {
                const int v = ctx->cells[(size_t)c1*nV+k];
                for (int t = vptr[v]; t < vptr[v+1]; t++)
                    if (vcells[t] >= c1) nbr.push_back(vcells[t]);
            }
            std::sort(nbr.begin(), nbr.end());
            for (size_t t = 0; t < nbr.size();) {
                size_t u = t;
                while (u < nbr.size() && nbr[u] == nbr[t]) u++;
                const int common = (nbr[t] == c1) ? nV : (int)(u-t);
                if (common < 1 || common > nV) return fail(ctx, PNL_ERR_INVALID, "degenerate cell pair (%d,%d)", c1, nbr[t]);
                // which cell is cellNo1 of a touching pair decides the orientation of its singular rule (NA:1386-1396: c1 <= c2 in
                // the CALLER's numbering): renumbered cells keep it (pnl_set_cell_order)
                if (!ctx->cell_orig.empty() && ctx->cell_orig[c1] > ctx->cell_orig[nbr[t]])
                    ctx->spairs_host[common-1].push_back(make_int2(nbr[t], c1));
                else
                    ctx->spairs_host[common-1].push_back(make_int2(c1, nbr[t]));
                t = u;
            }
        }
    }
    return PNL_OK;
}

// class of a cell pair / cell-facet pair (Kernel.evalParams at the two centres, NO:509-513)
static int class_cc(const pnl_context *ctx, int c1, int c2) {
    return ctx->nlab ? ctx->cls_of[(size_t)ctx->cell_labels[c1]*ctx->nlab+ctx->cell_labels[c2]] : 0;
}
static int class_cf(const pnl_context *ctx, int c1, int f) {
    return ctx->nlab ? ctx->cls_of[(size_t)ctx->cell_labels[c1]*ctx->nlab+ctx->facet_labels[f]] : 0;
}

// the touching cell pairs of every class on the device
static int upload_touching_pairs(pnl_context *ctx) {
    int rc;
    const int ncls = (int)ctx->cls.size();
    for (int s = 0; s < 3; s++)
        for (int k = 0; k < ncls; k++) {
            std::vector<int2> mine;
            for (const int2 &pr : ctx->spairs_host[s])
                if (class_cc(ctx, pr.x, pr.y) == k) mine.push_back(pr);
            ctx->cls[k]->n_spairs[s] = (int)mine.size();
            if ((rc = upload(ctx, ctx->cls[k]->b_spairs[s], mine.data(), mine.size()))) return rc;
            ctx->cls[k]->n_spairs1[s] = 0;
            if (ctx->nonsym) {
                // second orientation (swapCells, NA:1418): the pair (c2, c1) with the class of (label c2, label c1); identical
                // pairs are visited once
                std::vector<int2> swapped;
                for (const int2 &pr : ctx->spairs_host[s])
                    if (pr.x != pr.y && class_cc(ctx, pr.y, pr.x) == k) swapped.push_back(make_int2(pr.y, pr.x));
                ctx->cls[k]->n_spairs1[s] = (int)swapped.size();
                if ((rc = upload(ctx, ctx->cls[k]->b_spairs1[s], swapped.data(), swapped.size()))) return rc;
            }
        }
    return PNL_OK;
}

// boundary facets: vertex tables, touching (cell, facet) pairs per class, per-facet geometry
static int boundary_facets(pnl_context *ctx, const CellTables &F) {
    int rc;
    const int dim = F.dim, ncls = (int)ctx->cls.size(), nlab = ctx->nlab;
    const std::vector<int> &vptr = F.vptr, &vcells = F.vcells;
    for (int k = 0; k < ncls; k++) ctx->cls[k]->n_bpairs[0] = ctx->cls[k]->n_bpairs[1] = 0;
    if (!ctx->have_boundary) return PNL_OK;
    if (nlab > 0 && (int)ctx->facet_labels.size() != ctx->nb) return fail(ctx, PNL_ERR_STATE, "facet labels do not match the boundary");
    const int nF = dim, nb = ctx->nb;
    std::vector<int32_t> bvid((size_t)nF*nb);
    std::vector<double> bv((size_t)nF*dim*nb);
    std::vector<int2> bp[2];
    for (int f = 0; f < nb; f++) {
        for (int k = 0; k < nF; k++) {
            const int v = ctx->bcells[(size_t)f*nF+k];
            if (v < 0 || v >= ctx->nv) return fail(ctx, PNL_ERR_INVALID, "facet %d references vertex %d", f, v);
            bvid[(size_t)k*nb+f] = v;
            for (int d = 0; d < dim; d++) bv[(size_t)(k*dim+d)*nb+f] = ctx->vertices[(size_t)v*dim+d];
        }
    }
    {
        std::vector<int> nbr;
        for (int f = 0; f < nb; f++) {
            nbr.clear();
            for (int k = 0; k < nF; k++) {
                const int v = ctx->bcells[(size_t)f*nF+k];
                for (int t = vptr[v]; t < vptr[v+1]; t++) nbr.push_back(vcells[t]);
            }
            std::sort(nbr.begin(), nbr.end());
            for (size_t t = 0; t < nbr.size();) {
                size_t u = t;
                while (u < nbr.size() && nbr[u] == nbr[t]) u++;
                const int common = (int)(u-t);
                if (common > nF) return fail(ctx, PNL_ERR_INVALID, "degenerate cell/facet pair");
                bp[common-1].push_back(make_int2(nbr[t], f));
                t = u;
            }
        }
    }
    for (int s = 0; s < 2; s++)
        for (int k = 0; k < ncls; k++) {
            std::vector<int2> mine;
            for (const int2 &pr : bp[s])
                if (class_cf(ctx, pr.x, pr.y) == k) mine.push_back(pr);
            ctx->cls[k]->n_bpairs[s] = (int)mine.size();
            if ((rc = upload(ctx, ctx->cls[k]->b_bpairs[s], mine.data(), mine.size()))) return rc;
        }
    if (nlab > 0 && (rc = upload(ctx, ctx->b_blabel, ctx->facet_labels.data(), ctx->facet_labels.size()))) return rc;
    if ((rc = upload(ctx, ctx->b_bvid, bvid.data(), bvid.size()))) return rc;
    if ((rc = upload(ctx, ctx->b_bv, bv.data(), bv.size()))) return rc;
    // per-facet geometry used by every (cell, facet) pair: NO:1049-1055 normal, get_h_surface_simplex
    std::vector<double> geo((size_t)(2*dim+3)*nb, 0.);
    for (int f = 0; f < nb; f++) {
        double len = 1.;
        for (int d = 0; d < dim; d++) {
            double sum = 0.;
            for (int k = 0; k < nF; k++) sum += bv[(size_t)(k*dim+d)*nb+f];
            geo[(size_t)d*nb+f] = sum*(1./nF);
        }
        if (dim == 2) {
            double n0 = bv[(size_t)(1*dim+1)*nb+f]-bv[(size_t)(0*dim+1)*nb+f];
            double n1 = bv[(size_t)(0*dim+0)*nb+f]-bv[(size_t)(1*dim+0)*nb+f];
            const double inv = 1./std::sqrt(n0*n0+n1*n1);
            geo[(size_t)(dim+0)*nb+f] = n0*inv;
            geo[(size_t)(dim+1)*nb+f] = n1*inv;
            const double dx = bv[(size_t)2*nb+f]-bv[(size_t)0*nb+f], dy = bv[(size_t)3*nb+f]-bv[(size_t)1*nb+f];
            len = std::sqrt(dx*dx+dy*dy);
        }
        geo[(size_t)(2*dim)*nb+f] = len;
        geo[(size_t)(2*dim+1)*nb+f] = std::fabs(std::log(len/ctx->H0));
        geo[(size_t)(2*dim+2)*nb+f] = std::log(len);
    }
    return upload(ctx, ctx->b_bgeo, geo.data(), geo.size());
}

// per-block aggregates for the host-side tile classification (uniform tiles); clog: rows 0 / 1 / 2 of DevProblem::clog
static void block_aggregates(pnl_context *ctx, const CellTables &F, const std::vector<double> &clog) {
    const int dim = F.dim, nV = F.nV, nc = F.nc, T = F.T, nblocks = F.nblocks, ncp = F.ncp;
    const std::vector<double> &cellv = F.cellv, &ccen = F.ccen, &ch = F.ch;
    ctx->blocks.assign(nblocks, pnl_context::BlockAgg{0., 0., 0., 0., 0., 0., 0., false, 0., 0., 0.});
    for (int b = 0; b < nblocks; b++) {
        auto &B = ctx->blocks[b];
        const int c0 = b*T, c1 = std::min(nc, (b+1)*T);
        B.full = (c1-c0 == T);
        double sx = 0., sy = 0.;
        for (int c = c0; c < c1; c++) { sx += ccen[c]; if (dim == 2) sy += ccen[(size_t)ncp+c]; }
        B.cx = sx/(c1-c0); B.cy = sy/(c1-c0);
        B.rad = 0.; B.hmax = 0.; B.hmin = 1e300; B.Lmin = 1e300; B.Lmax = -1e300;
        for (int c = c0; c < c1; c++) {
            const double dx = ccen[c]-B.cx, dy = dim == 2 ? ccen[(size_t)ncp+c]-B.cy : 0.;
            B.rad = std::max(B.rad, std::sqrt(dx*dx+dy*dy));
            B.hmax = std::max(B.hmax, ch[c]);
            B.hmin = std::min(B.hmin, ch[c]);
            B.Lmin = std::min(B.Lmin, clog[(size_t)ncp+c]);
            B.Lmax = std::max(B.Lmax, clog[(size_t)ncp+c]);
        }
        // the same ball around the block in the coordinates of the interaction transform, vertices included
        B.tcx = B.cx; B.tcy = B.cy; B.trad = B.rad+B.hmax;
        if (ctx->have_xform && dim == 2) {
            double tx = 0., ty = 0.;
            int nvb = 0;
            for (int c = c0; c < c1; c++) for (int k = 0; k < nV; k++) { tx += cellv[(size_t)(k*dim)*ncp+c]; ty += cellv[(size_t)(k*dim+1)*ncp+c]; nvb++; }
            B.tcx = tx/nvb; B.tcy = ty/nvb; B.trad = 0.;
            for (int c = c0; c < c1; c++) for (int k = 0; k < nV; k++) {
                const double dx = cellv[(size_t)(k*dim)*ncp+c]-B.tcx, dy = cellv[(size_t)(k*dim+1)*ncp+c]-B.tcy;
                B.trad = std::max(B.trad, std::sqrt(dx*dx+dy*dy));
            }
        }
    }
    ctx->tiles_cached.clear(); ctx->tiles_cb = -1;
}

// uploads: vertices, labels, the padded cell tables, ln h and the radii, the per-block DoF lists
static int upload_cell_tables(pnl_context *ctx, const CellTables &F) {
    int rc;
    const int dim = F.dim, nV = F.nV, nc = F.nc, ncp = F.ncp, nlab = ctx->nlab;
    const std::vector<double> &ccen = F.ccen, &ch = F.ch;
    if ((rc = upload(ctx, ctx->b_vertices, ctx->vertices.data(), ctx->vertices.size()))) return rc;
    if (nlab > 0) {
        std::vector<int32_t> cl(ncp, 0);
        std::copy(ctx->cell_labels.begin(), ctx->cell_labels.end(), cl.begin());
        if ((rc = upload(ctx, ctx->b_clabel, cl.data(), cl.size()))) return rc;
        if ((rc = upload(ctx, ctx->b_clsof, ctx->cls_of.data(), ctx->cls_of.size()))) return rc;
    }
    if ((rc = upload(ctx, ctx->b_cellv, F.cellv.data(), F.cellv.size()))) return rc;
    if ((rc = upload(ctx, ctx->b_ccen, ccen.data(), ccen.size()))) return rc;
    if ((rc = upload(ctx, ctx->b_cvol, F.cvol.data(), F.cvol.size()))) return rc;
    if ((rc = upload(ctx, ctx->b_ch, ch.data(), ch.size()))) return rc;
    {
        std::vector<double> clog((size_t)3*ncp, 0.);
        for (int c = 0; c < ncp; c++) { clog[c] = std::log(ch[c]); clog[(size_t)ncp+c] = std::fabs(std::log(ch[c]/ctx->H0)); }
        // third row: the largest distance centre -- vertex of the cell in mesh coordinates, rounded up.  Two cells that share a
        // vertex have their centres within the sum of these radii: the tile kernels compare vertex ids only for such pairs
        for (int c = 0; c < nc; c++) {
            double r2 = 0.;
            for (int k = 0; k < nV; k++) {
                const int v = ctx->cells[(size_t)c*nV+k];
                double t2 = 0.;
                for (int d = 0; d < dim; d++) { const double t = ctx->vertices[(size_t)v*dim+d]-ccen[(size_t)d*ncp+c]; t2 += t*t; }
                r2 = std::max(r2, t2);
            }
            clog[(size_t)2*ncp+c] = std::sqrt(r2)*(1.+1e-5);
        }
        if ((rc = upload(ctx, ctx->b_clog, clog.data(), clog.size()))) return rc;
        block_aggregates(ctx, F, clog);
    }
    if ((rc = upload(ctx, ctx->b_cvid, F.cvid.data(), F.cvid.size()))) return rc;
    if ((rc = upload(ctx, ctx->b_cdof, F.cdof.data(), F.cdof.size()))) return rc;
    if ((rc = upload(ctx, ctx->b_cslot, F.cslot.data(), F.cslot.size()))) return rc;
    if ((rc = upload(ctx, ctx->b_blk_ndof, F.blk_ndof.data(), F.blk_ndof.size()))) return rc;
    if ((rc = upload(ctx, ctx->b_blk_dofs, F.blk_dofs.data(), F.blk_dofs.size()))) return rc;
    return PNL_OK;
}

// block-slot storage (pnl_tile2.h): padded column offsets, row offsets, the copies (block, slot) of every DoF
static int upload_slot_tables(pnl_context *ctx, const CellTables &F) {
    int rc;
    const int nblocks = F.nblocks;
    const std::vector<std::vector<int>> &lists = F.lists;
    const std::vector<int32_t> &blk_ndof = F.blk_ndof;
    std::vector<int32_t> colbase(nblocks+1, 0);
    for (int b = 0; b < nblocks; b++) colbase[b+1] = colbase[b]+((blk_ndof[b]+7) & ~7);
    const int S = colbase[nblocks];
    std::vector<long long> rowoff(nblocks, 0);
    long long run = 0;
    for (int a = 0; a < nblocks; a++) { rowoff[a] = run; run += (long long)blk_ndof[a]*(S-colbase[a]); }
    ctx->slot_S = S; ctx->slot_total = run;
    std::vector<int32_t> cpoff(ctx->N+1, 0);
    for (int b = 0; b < nblocks; b++) for (int g : lists[b]) cpoff[g+1]++;
    for (int g = 0; g < ctx->N; g++) cpoff[g+1] += cpoff[g];
    std::vector<int2> cp(cpoff[ctx->N]);
    std::vector<int32_t> fillp(cpoff.begin(), cpoff.end()-1);
    std::vector<long long> cprow(cp.size());
    for (int b = 0; b < nblocks; b++)
        for (size_t r = 0; r < lists[b].size(); r++) {
            const int k = fillp[lists[b][r]]++;
            cp[k] = make_int2(b, colbase[b]+(int)r);
            cprow[k] = rowoff[b]+(long long)r*(S-colbase[b])-colbase[b];
        }
    if ((rc = upload(ctx, ctx->b_cprow, cprow.data(), cprow.size()))) return rc;
    if ((rc = upload(ctx, ctx->b_scolbase, colbase.data(), colbase.size()))) return rc;
    if ((rc = upload(ctx, ctx->b_srowoff, rowoff.data(), rowoff.size()))) return rc;
    if ((rc = upload(ctx, ctx->b_cpoff, cpoff.data(), cpoff.size()))) return rc;
    if ((rc = upload(ctx, ctx->b_cpslot, cp.data(), cp.size()))) return rc;
    // the same tables packed per range of 32 DoFs (k_fold_mirror loads a range with one round trip): header (count) +
    // PNL_FOLD_TAB entries (row offset, block << 5 | local DoF, slot column); ranges with more copies use the lists above
    const int nranges = (ctx->N+31)/32;
    std::vector<FoldEntry> tab((size_t)nranges*(PNL_FOLD_TAB+1));
    for (int q = 0; q < nranges; q++) {
        FoldEntry *e = &tab[(size_t)q*(PNL_FOLD_TAB+1)];
        const int g0 = cpoff[q*32], g1 = cpoff[std::min(ctx->N, q*32+32)];
        e[0].off = g1-g0; e[0].ar = 0; e[0].cy = 0;
        if (g1-g0 > PNL_FOLD_TAB) continue;
        for (int I = q*32; I < std::min(ctx->N, q*32+32); I++)
            for (int g = cpoff[I]; g < cpoff[I+1]; g++) {
                FoldEntry &x = e[1+g-g0];
                x.off = cprow[g]; x.ar = (cp[g].x << 5) | (I-q*32); x.cy = cp[g].y;
            }
    }
    return upload(ctx, ctx->b_foldtab, tab.data(), tab.size());
}

// filling DevProblem
static void fill_problem(pnl_context *ctx, const CellTables &F) {
    const int dim = F.dim, dpe = F.dpe, nc = F.nc, ncp = F.ncp, nblocks = F.nblocks, nU = ctx->nU, nlab = ctx->nlab;
    DevProblem &P = ctx->P;
    P.dim = dim; P.dpe = dpe; P.nc = nc; P.ncp = ncp; P.N = ctx->N; P.dpv = ctx->dpv; P.dped = ctx->dped; P.nb = ctx->nb;
    P.H0 = ctx->H0;
    P.cellv = (const double*)ctx->b_cellv.p; P.ccen = (const double*)ctx->b_ccen.p;
    P.cvol = (const double*)ctx->b_cvol.p; P.ch = (const double*)ctx->b_ch.p; P.clog = (const double*)ctx->b_clog.p;
    P.cvid = (const int*)ctx->b_cvid.p; P.cdof = (const int*)ctx->b_cdof.p; P.cslot = (const short*)ctx->b_cslot.p;
    P.blk_ndof = (const int*)ctx->b_blk_ndof.p; P.blk_dofs = (const int*)ctx->b_blk_dofs.p;
    P.blk_stride = nU; P.nblocks = nblocks;
    P.perm_table = (const int*)ctx->b_perm.p;
    P.bvid = (const int*)ctx->b_bvid.p; P.bv = (const double*)ctx->b_bv.p; P.bgeo = (const double*)ctx->b_bgeo.p;
    P.counters = (unsigned long long*)ctx->b_counters.p;
    P.nlab = nlab; P.cur_class = -1; P.orient = 0; P.pad2 = 0; P.idfac = 1.;
    P.clabel = (const int*)ctx->b_clabel.p; P.blabel = (const int*)ctx->b_blabel.p; P.cls_of = (const int*)ctx->b_clsof.p;
}

// Build everything derived from mesh + DoF map: padded SoA cell arrays, per-block unique DoF lists,
// touching cell pairs, touching cell/facet pairs.
static int finalize(pnl_context *ctx) {
    if (!ctx->dirty) return PNL_OK;
    if (!ctx->have_mesh || !ctx->have_dofs) return fail(ctx, PNL_ERR_STATE, "mesh and DoF map must be uploaded first");
    const int dim = ctx->dim, nV = dim+1, nc = ctx->nc, dpe = ctx->dpe;
    if (!((dim == 2 && (dpe == 1 || dpe == 3 || dpe == 6)) || (dim == 1 && dpe >= 1 && dpe <= 4)))          // 2D: P0, P1, P2; 1D: P0 .. P3
        return fail(ctx, PNL_ERR_UNSUPPORTED, "unsupported (dim=%d, dofs_per_element=%d)", dim, dpe);
    // P2 blocks hold about twice the DoFs per cell: half the cells per block keep the LDS sub-block in range
    const int T = ctx->tile = (dpe == 6 || (dim == 1 && dpe >= 3)) ? TILE_P2 : TILE_P1;
    const int nblocks = ctx->nblocks = (nc+T-1)/T;
    const int ncp = ctx->ncp = nblocks*T;
    CellTables F;
    F.dim = dim; F.nV = nV; F.nc = nc; F.dpe = dpe; F.T = T; F.nblocks = nblocks; F.ncp = ncp;
    tile_order_drop(ctx);
    int rc;
    if ((rc = padded_cell_tables(ctx, F))) return rc;
    block_dofs(ctx, F);
    // permuted copies for the tile kernels: built and uploaded by pnl_tile_order_ready once the search has finished; 2D P1 also the
    // lane layout of the uniform-tile kernels, which reads the slots of the blocks (so the job starts behind block_dofs)
    ctx->have_tile_order = false;
    ctx->uni_lanes_up = -1;
    if (dpe == nV && dim == 2) start_tile_order_search(ctx, F);
    if ((rc = touching_cell_pairs(ctx, F))) return rc;
    if (ctx->nlab > 0 && (int)ctx->cell_labels.size() != nc) return fail(ctx, PNL_ERR_STATE, "cell labels do not match the mesh");
    if ((rc = upload_touching_pairs(ctx))) return rc;
    if ((rc = boundary_facets(ctx, F))) return rc;
    if ((rc = upload_cell_tables(ctx, F))) return rc;
    if ((rc = upload_slot_tables(ctx, F))) return rc;
    if ((rc = upload(ctx, ctx->b_perm, ctx->perm_table.data(), ctx->perm_table.size()))) return rc;
    const bool fresh_counters = !ctx->b_counters.p;
    if ((rc = ensure(ctx, ctx->b_counters, sizeof(unsigned long long)*PNL_NCOUNTERS))) return rc;
    // pnl_synchronize reads the loss counters of a context that may never assemble (an operator installed by pnl_h2_set)
    if (fresh_counters) HIPCHK(ctx, hipMemset(ctx->b_counters.p, 0, sizeof(unsigned long long)*PNL_NCOUNTERS));
    if ((rc = ensure(ctx, ctx->b_D, sizeof(double)*(size_t)ncp*(dpe*(dpe+1)/2)))) return rc;
    fill_problem(ctx, F);
    ctx->dirty = false;
    return PNL_OK;
}

// Tables of pnl_pow_tab for x^exponent * scale (long double on the host, rounded once):  x = 2^k m, m in [1, 2), j = top seven
// fraction bits of m, c_j = 1 / fl(1 / (1 + (j + 1/2) / 128)), u = m fl(1/c_j) - 1 (one FMA, |u| <= 2^-8):
//   x^e = 2^(e k) c_j^e (1 + u)^e.
// also_fast: tables for an exponent -qm/4 as well -- a launch over the tiles of SEVERAL order classes runs the KT == 0 kernels for
// all of them, and a class without tables falls into the general branch there (exp(e ln x) behind the per-lane horizon test)
bool pow_table_values(const DevKernel &k, bool also_fast, std::vector<double> &tab) {
    if (k.ktype != PNL_FRACTIONAL || (k.fast && !also_fast) || pnl_tune("PNL_NO_POWTAB")) return false;
    tab.assign(PNL_POW_TAB_DOUBLES, 0.);
    for (int j = 0; j < 128; j++) {
        const double invc = (double)(1.L/(1.L+((long double)j+0.5L)/128.L));
        const long double c = 1.L/(long double)invc;
        tab[j] = invc;
        tab[128+j] = (double)((long double)k.scale*powl(c, (long double)k.exponent));
        tab[256+j] = (double)exp2l((long double)k.exponent*(long double)(j-96));
    }
    return true;
}

const double *pnl_pow_table(pnl_context *ctx, const DevKernel &k, bool also_fast) {
    if (k.ktype != PNL_FRACTIONAL || (k.fast && !also_fast) || pnl_tune("PNL_NO_POWTAB")) return nullptr;
    for (auto *t : ctx->powtabs) if (t->exponent == k.exponent && t->scale == k.scale) return (const double*)t->buf.p;
    std::vector<double> tab;
    if (!pow_table_values(k, also_fast, tab)) return nullptr;
    auto *t = new pnl_context::PowTab;
    t->exponent = k.exponent; t->scale = k.scale;
    if (upload(ctx, t->buf, tab.data(), tab.size()) != PNL_OK) { delete t; return nullptr; }
    ctx->powtabs.push_back(t);
    return (const double*)t->buf.p;
}

void pnl_refresh_tables(pnl_context *ctx) {
    DevProblem &P = ctx->P;
    P.k = to_dev(ctx->C().kern[0], ctx->dim);
    P.bk = to_dev(ctx->C().kern[1], ctx->dim);
    P.bkn = to_dev_bkn(ctx->C().kern[1], ctx->dim);     // n.(y-x)/|y-x| * Gamma_b(|x-y|^2), the normalisation folded in
    P.qo = to_dev(ctx->C().form[0]);
    P.bqo = to_dev(ctx->C().form[1]);
    P.qmax = ctx->qmax;
    P.off = (const int*)ctx->b_off.p; P.bary = (const double*)ctx->b_bary.p; P.w = (const double*)ctx->b_w.p;
    P.phi = (const double*)ctx->b_phi.p; P.foff = (const int*)ctx->b_foff.p; P.fbary = (const double*)ctx->b_fbary.p;
    P.fw = (const double*)ctx->b_fw.p;
    P.tt_n = (const int*)ctx->b_ttn.p; P.tt_off = (const int*)ctx->b_ttoff.p; P.tt_tab = (const double*)ctx->b_tttab.p;
    P.tt_wphi = (const double*)ctx->b_ttwphi.p;
    P.tt_wphif = (const double*)ctx->b_ttwphif.p;
    for (int s = 0; s < 3; s++) {
        P.sNodes[s] = (const double*)ctx->C().b_sn[s].p; P.sW[s] = (const double*)ctx->C().b_sw[s].p; P.sPsi[s] = (const double*)ctx->C().b_sp[s].p;
    }
    for (int s = 0; s < 2; s++) {
        P.bNodes[s] = (const double*)ctx->C().b_bn[s].p; P.bW[s] = (const double*)ctx->C().b_bw[s].p; P.bPhi[s] = (const double*)ctx->C().b_bp[s].p;
    }
    for (int s = 0; s < 3; s++) { P.sM[s] = ctx->C().sM[s]; P.sRows[s] = ctx->C().sRows[s]; }
    for (int s = 0; s < 2; s++) P.bM[s] = ctx->C().bM[s];
    P.sFac = ctx->C().sFac; P.bFac = ctx->C().bFac;
    P.cur_class = ctx->nlab > 0 ? ctx->cur : -1;
    // non-symmetric order table: two passes per class with half the kernel each (see DevProblem::orient)
    P.orient = ctx->nonsym ? ctx->orient : 0;
    P.idfac = ctx->nonsym ? 2. : 1.;
    if (ctx->nonsym) P.k.scale *= 0.5;
    P.k.ptab = pnl_pow_table(ctx, P.k);                      // after the last change of the scale: the tables carry it
}

static int check_ready(pnl_context *ctx) {
    for (auto *c : ctx->cls)
        if (!c->have_kernel[0] || !c->have_form[0] || !ctx->have_rules)
            return fail(ctx, PNL_ERR_STATE, "kernel, order formula and distant rules must be set (for every class) before assembling");
    return PNL_OK;
}

// the launching units: see pnl_context.h
int pnl_assembly_ready(pnl_context *ctx) {
    int rc;
    if ((rc = check_ready(ctx))) return rc;
    return finalize(ctx);
}
int pnl_assembly_prepare(pnl_context *ctx) {
    int rc;
    if ((rc = pnl_assembly_ready(ctx))) return rc;
    pnl_refresh_tables(ctx);
    return PNL_OK;
}

// =================================================================================================
// Are all cell pairs of the tile (block a, block b) distant pairs of ONE quadrature order q <= qlimit?  Returns q or 0.
// Conservative bounds on the order formula (FL2:622-642 / FL1:234-253)
//   order = max(ceil f(1,2), ceil f(2,1), 2),  f(self, other) = (c0 + a L_other + b max(L_self, L_other) - e ln(d/h_other)) / (max(ln(d/h_self), 0) + den0)
// over the tile: the distance of the cell centres lies in [dmin, dmax] = |centre_a - centre_b| -+ (rad_a + rad_b), h in
// [hmin, hmax] and L = |ln(h/H0)| in [Lmin, Lmax] per block.  f <= num_max/den_min for both roles gives order <= q, and
// f >= num_min/den_max > q-1 for ONE role (for all pairs of the tile) gives order >= q.  dmin > hmax_a + hmax_b also rules
// out shared vertices (a vertex is closer than 2/3 h to its cell's centre).  Anything not provably uniform goes to the
// general kernel, whose per-pair formula decides.
int pnl_tile_uniform_order(const pnl_context *ctx, const pnl_order_formula &F, int ta, int tb, int qlimit) {
    if (ta == tb) return 0;
    const auto &A = ctx->blocks[ta], &B = ctx->blocks[tb];
    if (!A.full || !B.full || !(F.e >= 0.) || !(F.den0 > 0.)) return 0;
    const double dx = A.cx-B.cx, dy = A.cy-B.cy, dc = std::sqrt(dx*dx+dy*dy);
    const double dmin = dc-A.rad-B.rad, dmax = dc+A.rad+B.rad;
    if (!(dmin > A.hmax+B.hmax)) return 0;
    typedef pnl_context::BlockAgg Agg;
    auto upper = [&](const Agg &S, const Agg &O, double q) {       // f(S, O) <= q for every pair
        const double l_self = std::log(dmin/S.hmax), n_other = std::log(dmin/O.hmax);      // both > 0
        const double aL = std::max(F.a*O.Lmin, F.a*O.Lmax);
        const double bL = std::max(F.b*std::max(S.Lmin, O.Lmin), F.b*std::max(S.Lmax, O.Lmax));
        const double num = F.c0+aL+bL-F.e*n_other, den = l_self+F.den0;
        return num <= q*den*(1.-1e-9)-1e-9;
    };
    auto lower = [&](const Agg &S, const Agg &O, double q) {       // f(S, O) > q for every pair
        const double l_self = std::log(dmax/S.hmin), n_other = std::log(dmax/O.hmin);
        const double aL = std::min(F.a*O.Lmin, F.a*O.Lmax);
        const double bL = std::min(F.b*std::max(S.Lmin, O.Lmin), F.b*std::max(S.Lmax, O.Lmax));
        const double num = F.c0+aL+bL-F.e*n_other, den = l_self+F.den0;
        return den > 0. && num >= q*den*(1.+1e-9)+1e-9;
    };
    for (int q = 2; q <= qlimit; q++)
        if (upper(A, B, q) && upper(B, A, q)) {
            if (q == 2) return 2;
            return (lower(A, B, q-1) || lower(B, A, q-1)) ? q : 0;
        }
    return 0;
}

// ---- options (pnl_context.h: pnl_tune) --------------------------------------------------------------------------------------
namespace {
std::mutex g_opt_mutex;
// values are interned and never freed: a pointer pnl_tune() handed out stays valid while another thread sets or erases the option
// (the set of distinct values a process names is small)
std::map<std::string, const std::string*> g_options;
std::deque<std::string> g_option_values;
// the options pnl_set_option accepts, all of them: the hooks through which the parity tests reach the alternative code paths, and
// the diagnostics.  Every name is read by a pnl_tune call with the literal name somewhere in csrc/ (tests/test_abi.py checks both directions)
const char *const k_product_options[] = {
    "PNL_WL_FRAC",          // tests: work-list capacity as a fraction of the pairs, floor 64 entries (overflow must fail the call)
    "PNL_FH_NOTILES",       // reference path: finite-horizon pairs through the pair lists, not the tile kernel
    "PNL_NO_POWTAB",        // reference path: general power by exp / log instead of the tables
    "PNL_VERBOSE",          // diagnostics: launch shapes and plan statistics on stderr
    "PNL_PLAN_TIMING",      // diagnostics: times of the pattern planner's phases on stderr
    "PNL_PLAN_THREADS",     // host threads of the planner
    "PNL_BND_OLD",          // reference path: boundary term by k_boundary_distant instead of the tiled kernel
    "PNL_NO_OVERLAP",       // profiling: every phase on the caller's stream, one after the other (per-kernel times that add up)
    "PNL_NO_FORK",          // profiling: the order classes one after the other, no side streams
    "PNL_TILE_WGS",         // tests: at most this many workgroups of a persistent tile kernel (every workgroup then walks many
                            // tiles at test sizes: the pipelined tile loops against the oracle)
    "PNL_UNI_GENERIC",      // reference path: uniform P1 tiles without the structured-rule evaluators
    "PNL_UNI_CHECKED",      // tests: no uniform tile skips the per-pair validity test
    "PNL_UNI_LANES",        // lane layout of the uniform P1 tiles: 0 identity, 1 searched (default), 2 random
    "PNL_MIXED_GENERIC",    // reference path: mixed tiles without the structured-rule evaluators
    "PNL_MIXED_UNSETTLED",  // reference path: every mixed tile through the classifying kernel
    "PNL_SETTLED_CODES",    // reference path: settled tiles by their pair codes, not by the plan's pair lists
};
}  // namespace

const char *pnl_tune(const char *name) {
    {
        std::lock_guard<std::mutex> lk(g_opt_mutex);
        auto it = g_options.find(name);
        if (it != g_options.end()) return it->second->c_str();
    }
    return nullptr;
}

extern "C" {

const char *pnl_version(void) {
    return "pnl_hip 0.1 (gfx950)";
}

int pnl_set_option(const char *name, const char *value) {
    if (!name) return PNL_ERR_INVALID;
    bool known = false;
    for (const char *k : k_product_options) known = known || std::strcmp(k, name) == 0;
    if (!known) return PNL_ERR_UNSUPPORTED;
    std::lock_guard<std::mutex> lk(g_opt_mutex);
    if (value) {
        const std::string *v = nullptr;
        for (const std::string &have : g_option_values) if (have == value) { v = &have; break; }
        if (!v) { g_option_values.emplace_back(value); v = &g_option_values.back(); }     // deque: earlier elements do not move
        g_options[name] = v;
    } else g_options.erase(name);
    return PNL_OK;
}

int pnl_create(int device_id, pnl_context **out) {
    if (!out) return PNL_ERR_INVALID;
    *out = nullptr;
    int ndev = 0;
    hipError_t e0;
    auto hiperr = [](const char *what, hipError_t e) { fprintf(stderr, "[pnl] pnl_create: %s failed: %s\n", what, hipGetErrorString(e)); return PNL_ERR_HIP; };
    if ((e0 = hipGetDeviceCount(&ndev)) != hipSuccess || ndev <= 0) return hiperr("hipGetDeviceCount", e0);
    if (device_id < 0 || device_id >= ndev) return PNL_ERR_INVALID;
    if ((e0 = hipSetDevice(device_id)) != hipSuccess) return hiperr("hipSetDevice", e0);
    pnl_context *ctx = new pnl_context();
    ctx->device = device_id;
    if ((e0 = hipStreamCreate(&ctx->own_stream)) != hipSuccess) { delete ctx; return hiperr("hipStreamCreate", e0); }
    ctx->stream = ctx->own_stream;
    for (auto &st : ctx->aux)
        if ((e0 = hipStreamCreateWithFlags(&st, hipStreamNonBlocking)) != hipSuccess) { delete ctx; return hiperr("hipStreamCreateWithFlags", e0); }
    if (hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming) != hipSuccess) { delete ctx; return PNL_ERR_HIP; }
    if (hipEventCreateWithFlags(&ctx->ev_fold, hipEventDisableTiming) != hipSuccess) { delete ctx; return PNL_ERR_HIP; }
    for (auto &e : ctx->ev_join)
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { delete ctx; return PNL_ERR_HIP; }
    for (auto &e : ctx->ev)
        if (hipEventCreate(&e) != hipSuccess) { delete ctx; return PNL_ERR_HIP; }
    std::memset(&ctx->P, 0, sizeof(ctx->P));
    ctx->cls.push_back(new pnl_context::ClassData());
    *out = ctx;
    return PNL_OK;
}

void pnl_destroy(pnl_context *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    for (auto &e : ctx->ev)
        if (e) (void)hipEventDestroy(e);
    for (auto &v : ctx->kev)
        for (auto &e : v)
            if (e) (void)hipEventDestroy(e);
    tile_order_drop(ctx);
    for (auto &st : ctx->aux) if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    if (ctx->ev_fold) (void)hipEventDestroy(ctx->ev_fold);
    for (auto *t : ctx->powtabs) delete t;
    ctx->powtabs.clear();
    for (auto &e : ctx->ev_join) if (e) (void)hipEventDestroy(e);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    for (auto *c : ctx->cls) delete c;
    delete ctx;
}

const char *pnl_error_string(pnl_context *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int pnl_set_stream(pnl_context *ctx, void *hip_stream) {
    if (!ctx) return PNL_ERR_INVALID;
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return PNL_OK;
}

// Entries beyond a work list's capacity and pairs whose quadrature order exceeds the uploaded tables are dropped by the
// kernels; the counters that tell (one fill counter per class pass, counter 5) are read here so that the loss fails the
// first call that waits for the assembly instead of going unnoticed.
static int check_overflow(pnl_context *ctx) {
    if (ctx->b_wlcount.p && ctx->wl_cap_each > 0) {
        unsigned wl[PNL_WL_SLOTS];
        const int n = std::min(ctx->run.wl_slots, PNL_WL_SLOTS);      // the slots in use; the copy takes one word at least, as it always has
        HIPCHK(ctx, hipMemcpy(wl, ctx->b_wlcount.p, sizeof(unsigned)*std::max(1, n), hipMemcpyDeviceToHost));
        for (int i = 0; i < n; i++)
            if (wl[i] > ctx->wl_cap_each)
                return fail(ctx, PNL_ERR_STATE, "work list overflow (pass %d): %u entries needed, capacity %u; the assembled operator is "
                            "incomplete", i, wl[i], ctx->wl_cap_each);
    }
    if (ctx->b_counters.p) {
        unsigned long long ov = 0;
        HIPCHK(ctx, hipMemcpy(&ov, (const unsigned long long*)ctx->b_counters.p+5, sizeof(ov), hipMemcpyDeviceToHost));
        if (ov) return fail(ctx, PNL_ERR_ORDER, "%llu pairs need a quadrature order beyond the uploaded tables (qmax=%d); the assembled "
                            "operator is incomplete", ov, ctx->qmax);
        HIPCHK(ctx, hipMemcpy(&ov, (const unsigned long long*)ctx->b_counters.p+7, sizeof(ov), hipMemcpyDeviceToHost));
        if (ov) return fail(ctx, PNL_ERR_STATE, "%llu entries of touching pairs have no row in the slab (pnl_set_row_slab needs the DoFs of the "
                            "cells touching the rank's cells)", ov);
    }
    return PNL_OK;
}

int pnl_synchronize(pnl_context *ctx) {
    if (!ctx) return PNL_ERR_INVALID;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return check_overflow(ctx);
}

int pnl_upload_mesh(pnl_context *ctx, int dim, int nv, const double *vertices, int nc, const int32_t *cells,
                    const double *vol, const double *h, double H0) {
    if (!ctx) return PNL_ERR_INVALID;
    if (dim != 1 && dim != 2) return fail(ctx, PNL_ERR_UNSUPPORTED, "dim=%d is not implemented", dim);
    if (nv <= 0 || nc <= 0 || !vertices || !cells || !vol || !h || !(H0 > 0.)) return fail(ctx, PNL_ERR_INVALID, "bad mesh arguments");
    ctx->dim = dim; ctx->nv = nv; ctx->nc = nc; ctx->H0 = H0;
    ctx->vertices.assign(vertices, vertices+(size_t)nv*dim);
    ctx->cells.assign(cells, cells+(size_t)nc*(dim+1));
    ctx->vol.assign(vol, vol+nc);
    ctx->h.assign(h, h+nc);
    ctx->cell_orig.clear();
    ctx->have_mesh = true;
    ctx->dirty = true;
    return PNL_OK;
}

int pnl_set_interaction_transform(pnl_context *ctx, int dim, const double *T) {
    if (!ctx) return PNL_ERR_INVALID;
    if (T && dim != 2) return fail(ctx, PNL_ERR_UNSUPPORTED, "interaction transform: 2D only");
    ctx->have_xform = T != nullptr;
    for (int i = 0; i < 4; i++) ctx->xform[i] = T ? T[i] : (i == 0 || i == 3 ? 1. : 0.);
    if (T && !(std::fabs(T[0]*T[3]-T[1]*T[2]) > 0.)) return fail(ctx, PNL_ERR_INVALID, "interaction transform is singular");
    ctx->dirty = true;
    return PNL_OK;
}

int pnl_set_cell_order(pnl_context *ctx, int nc, const int32_t *orig) {
    if (!ctx) return PNL_ERR_INVALID;
    if (!ctx->have_mesh) return fail(ctx, PNL_ERR_STATE, "upload the mesh first");
    if (orig && nc != ctx->nc) return fail(ctx, PNL_ERR_INVALID, "pnl_set_cell_order: %d cells expected", ctx->nc);
    if (orig) ctx->cell_orig.assign(orig, orig+nc); else ctx->cell_orig.clear();
    ctx->dirty = true;
    return PNL_OK;
}

int pnl_upload_dofmap(pnl_context *ctx, int dpe, int dofs_per_vertex, int dofs_per_edge, int num_dofs, const int32_t *dofs,
                      const int32_t *perm_table) {
    if (!ctx) return PNL_ERR_INVALID;
    if (!ctx->have_mesh) return fail(ctx, PNL_ERR_STATE, "upload the mesh first");
    if (dpe <= 0 || num_dofs <= 0 || !dofs || !perm_table) return fail(ctx, PNL_ERR_INVALID, "bad DoF map arguments");
    // NA:941: the local matrix must fit the mask type (256 bits in the reference)
    if ((2*dpe)*(2*dpe+1)/2 > 256) return fail(ctx, PNL_ERR_INVALID, "local matrix has more than 256 entries");
    ctx->dpe = dpe; ctx->dpv = dofs_per_vertex; ctx->dped = dofs_per_edge; ctx->N = num_dofs;
    ctx->dofs.assign(dofs, dofs+(size_t)ctx->nc*dpe);
    int nperm = 1;
    for (int k = 2; k <= ctx->dim+1; k++) nperm *= k;
    ctx->perm_table.assign(perm_table, perm_table+(size_t)nperm*dpe);
    ctx->have_dofs = true;
    ctx->dirty = true;
    return PNL_OK;
}

int pnl_set_classes(pnl_context *ctx, int nclasses, int num_labels, const int32_t *cell_labels, const int32_t *facet_labels,
                    const int32_t *cls_of) {
    if (!ctx) return PNL_ERR_INVALID;
    if (!ctx->have_mesh) return fail(ctx, PNL_ERR_STATE, "upload the mesh first");
    if (nclasses < 1 || nclasses > 64 || num_labels < 0 || (num_labels > 0 && (!cell_labels || !cls_of)))
        return fail(ctx, PNL_ERR_INVALID, "bad class arguments");
    for (int i = 0; i < num_labels*num_labels; i++)
        if (cls_of[i] < 0 || cls_of[i] >= nclasses) return fail(ctx, PNL_ERR_INVALID, "class table entry %d out of range", i);
    for (int c = 0; num_labels > 0 && c < ctx->nc; c++)
        if (cell_labels[c] < 0 || cell_labels[c] >= num_labels) return fail(ctx, PNL_ERR_INVALID, "label of cell %d out of range", c);
    for (auto *c : ctx->cls) delete c;
    ctx->cls.clear();
    for (int k = 0; k < nclasses; k++) ctx->cls.push_back(new pnl_context::ClassData());
    ctx->cur = 0;
    ctx->nlab = num_labels;
    ctx->cell_labels.assign(cell_labels, cell_labels+(num_labels > 0 ? ctx->nc : 0));
    ctx->cls_of.assign(cls_of, cls_of+(size_t)num_labels*num_labels);
    ctx->tiles_cached.clear(); ctx->tiles_forms.clear();
    ctx->nonsym = false;
    ctx->facet_labels.clear();
    if (num_labels > 0 && facet_labels && ctx->have_boundary) {
        for (int f = 0; f < ctx->nb; f++)
            if (facet_labels[f] < 0 || facet_labels[f] >= num_labels) return fail(ctx, PNL_ERR_INVALID, "label of facet %d out of range", f);
        ctx->facet_labels.assign(facet_labels, facet_labels+ctx->nb);
    }
    ctx->dirty = true;
    return PNL_OK;
}

int pnl_set_nonsymmetric(pnl_context *ctx, int on) {
    if (!ctx) return PNL_ERR_INVALID;
    if (on && ctx->nlab == 0) return fail(ctx, PNL_ERR_STATE, "pnl_set_classes with labels first: only a label table can be non-symmetric");
    ctx->nonsym = on != 0;
    ctx->dirty = true;
    ctx->tiles_cached.clear(); ctx->tiles_forms.clear();
    return PNL_OK;
}

int pnl_select_class(pnl_context *ctx, int k) {
    if (!ctx) return PNL_ERR_INVALID;
    if (k < 0 || k >= (int)ctx->cls.size()) return fail(ctx, PNL_ERR_INVALID, "class %d out of range", k);
    ctx->cur = k;
    return PNL_OK;
}

int pnl_set_kernel(pnl_context *ctx, int which, const pnl_kernel *k) {
    if (!ctx || !k || which < 0 || which > 1) return fail(ctx, PNL_ERR_INVALID, "bad kernel arguments");
    if (k->ktype < 0 || k->ktype > PNL_EXPONENTIAL_BOUNDARY) return fail(ctx, PNL_ERR_UNSUPPORTED, "kernel type %d is not implemented", k->ktype);
    if (!std::isinf(k->horizon2) && (k->interaction < 1 || k->interaction > 2 || !(k->horizon2 > 0.)))
        return fail(ctx, PNL_ERR_UNSUPPORTED, "finite horizon: interaction %d is not implemented (1 ball2_retriangulation, 2 ball2_barycenter)",
                    k->interaction);
    ctx->C().kern[which] = *k;
    ctx->C().have_kernel[which] = true;
    return PNL_OK;
}

int pnl_set_order_formula(pnl_context *ctx, int which, const pnl_order_formula *f) {
    if (!ctx || !f || which < 0 || which > 1) return fail(ctx, PNL_ERR_INVALID, "bad order-formula arguments");
    ctx->C().form[which] = *f;
    ctx->C().have_form[which] = true;
    return PNL_OK;
}

// rule blocks of the uniform-order tiles (2D, orders 2-4 with 3 or 6 points): bary[n][3], w[n], w phi[n][dpe],
// w phi_a phi_b[nd][n] (a <= b, row-major upper triangle)
static int upload_uniform_rule_blocks(pnl_context *ctx, int qmax, const int32_t *off, const double *bary, const double *w, const double *phi) {
    const int dpe = ctx->dpe;
    std::vector<double> uni;
    for (int q = 0; q < 5; q++) { ctx->uni_off[q] = -1; ctx->uni_np[q] = 0; }
    for (int q = 2; q <= 4 && q <= qmax && ctx->dim == 2; q++) {
        const int n = off[q+1]-off[q];
        if (n != 3 && n != 6) continue;
        ctx->uni_off[q] = (int)uni.size(); ctx->uni_np[q] = n;
        // point order of the block: P1 with three points of equal weight whose shape values are A + B delta(b, sigma(i)) for a
        // permutation sigma (the symmetric degree-2 rule) -> the points in the order sigma^-1, so that w phi_b(y_i) = A + B delta_bi
        std::vector<int> ord(n);
        for (int i = 0; i < n; i++) ord[i] = i;
        ctx->uni_struct[q] = false;
        if (n == 3 && dpe == 3) {
            int sig[3] = {-1, -1, -1};
            bool ok = w[off[q]] == w[off[q]+1] && w[off[q]] == w[off[q]+2];
            for (int i = 0; i < 3 && ok; i++) {
                const double *ph = &phi[((size_t)off[q]+i)*dpe];
                int big = 0;
                for (int b = 1; b < 3; b++) if (ph[b] > ph[big]) big = b;
                sig[i] = big;
                for (int b = 0; b < 3; b++)
                    ok = ok && ph[b] == (b == big ? phi[(size_t)off[q]*dpe+sig[0]] : phi[(size_t)off[q]*dpe+(sig[0]+1)%3]);
            }
            ok = ok && sig[0] != sig[1] && sig[0] != sig[2] && sig[1] != sig[2];
            if (ok) {
                for (int i = 0; i < 3; i++) ord[sig[i]] = i;
                ctx->uni_struct[q] = true;
            }
        }
        // six points in two orbits of three (the symmetric 6-point rules of degree 3 / 4): per orbit equal weights and shape values
        // A_o + B_o delta(b, sigma(i)) -> the points in the order orbit 0 (positions 0, 1, 2), orbit 1 (positions 0, 1, 2)
        if (n == 6 && dpe == 3) {
            int big[6], orb[6], norb = 0;
            double ow[2] = {0., 0.}, ohi[2] = {0., 0.}, olo[2] = {0., 0.};
            bool ok = true;
            for (int i = 0; i < 6 && ok; i++) {
                const double *ph = &phi[((size_t)off[q]+i)*dpe];
                // the distinguished coordinate of a point (x, x, 1 - 2 x): the one that differs from the other two
                int d = -1;
                if (ph[0] == ph[1] && ph[0] != ph[2]) d = 2;
                else if (ph[0] == ph[2] && ph[0] != ph[1]) d = 1;
                else if (ph[1] == ph[2] && ph[0] != ph[1]) d = 0;
                if (d < 0) { ok = false; break; }
                big[i] = d;
                const double hi = ph[d], lo = ph[(d+1)%3], wi = w[off[q]+i];
                int o = -1;
                for (int t = 0; t < norb; t++) if (ow[t] == wi && ohi[t] == hi && olo[t] == lo) o = t;
                if (o < 0) { if (norb == 2) { ok = false; break; } o = norb++; ow[o] = wi; ohi[o] = hi; olo[o] = lo; }
                orb[i] = o;
            }
            if (ok && norb == 2) {
                int seen[2][3] = {{0, 0, 0}, {0, 0, 0}};
                for (int i = 0; i < 6; i++) seen[orb[i]][big[i]]++;
                for (int o = 0; o < 2; o++) for (int d = 0; d < 3; d++) ok = ok && seen[o][d] == 1;
                if (ok) {
                    for (int i = 0; i < 6; i++) ord[3*orb[i]+big[i]] = i;
                    ctx->uni_struct[q] = true;
                }
            }
        }
        auto pt = [&](int i) { return (size_t)off[q]+ord[i]; };
        for (int i = 0; i < n; i++) for (int k2 = 0; k2 < 3; k2++) uni.push_back(bary[3*pt(i)+k2]);
        for (int i = 0; i < n; i++) uni.push_back(w[pt(i)]);
        for (int i = 0; i < n; i++) for (int a = 0; a < dpe; a++) uni.push_back(w[pt(i)]*phi[pt(i)*dpe+a]);
        for (int a = 0; a < dpe; a++)
            for (int b = a; b < dpe; b++)
                for (int i = 0; i < n; i++) uni.push_back(w[pt(i)]*phi[pt(i)*dpe+a]*phi[pt(i)*dpe+b]);
    }
    return upload(ctx, ctx->b_uni, uni.data(), uni.size());
}

int pnl_upload_distant_rules(pnl_context *ctx, int qmax, const int32_t *off, const double *bary, const double *w,
                             const double *phi, const int32_t *foff, const double *fbary, const double *fw) {
    if (!ctx) return PNL_ERR_INVALID;
    if (!ctx->have_dofs) return fail(ctx, PNL_ERR_STATE, "upload the DoF map first");
    if (qmax < 2 || qmax > PNL_MAXQ || !off || !bary || !w || !phi || !foff || !fbary || !fw)
        return fail(ctx, PNL_ERR_INVALID, "bad rule arguments (2 <= qmax <= %d)", PNL_MAXQ);
    const int total = off[qmax+1], ftotal = foff[qmax+1];
    int rc;
    ctx->rule_off.assign(off, off+qmax+2); ctx->frule_off.assign(foff, foff+qmax+2);
    if ((rc = upload(ctx, ctx->b_off, off, (size_t)qmax+2))) return rc;
    if ((rc = upload(ctx, ctx->b_bary, bary, (size_t)total*3))) return rc;
    if ((rc = upload(ctx, ctx->b_w, w, (size_t)total))) return rc;
    if ((rc = upload(ctx, ctx->b_phi, phi, (size_t)total*ctx->dpe))) return rc;
    if ((rc = upload(ctx, ctx->b_foff, foff, (size_t)qmax+2))) return rc;
    if ((rc = upload(ctx, ctx->b_fbary, fbary, (size_t)ftotal*2))) return rc;
    if ((rc = upload(ctx, ctx->b_fw, fw, (size_t)ftotal))) return rc;
    // pack the orders with 2, 3, 4, 6 or 7 points (the unrolled lane-per-pair variants) for the tile kernel's LDS copy
    {
        const int dpe = ctx->dpe, st = 4+dpe;
        std::vector<int32_t> tn(PNL_MAXQ+2, 0), to(PNL_MAXQ+2, 0);
        std::vector<double> tab, wphi;
        int npts = 0, nb = 0;
        // the tile kernel unrolls exactly two point counts (3 and 6 on triangles, 2 and 3 on intervals) and integrates the
        // other orders with at most PNL_GEN_MAXPTS points through a generic loop (list C)
        const int nA = ctx->dim == 2 ? 3 : 2, nB = ctx->dim == 2 ? 6 : 3;
        for (int q = 2; q <= qmax && q < 18; q++) {
            const int n = off[q+1]-off[q];
            const bool ok = (n == nA || n == nB || (n > 0 && n <= PNL_GEN_MAXPTS));
            const int npad = n;
            if (!ok || npts+npad > PNL_TT_MAXPTS) continue;
            tn[q] = n; to[q] = npts;
            for (int i = 0; i < npad; i++) {
                const size_t p = (size_t)off[q]+(i < n ? i : 0);
                const double wp = i < n ? w[p] : 0.;
                tab.push_back(bary[3*p]); tab.push_back(bary[3*p+1]); tab.push_back(bary[3*p+2]); tab.push_back(wp);
                for (int a = 0; a < dpe; a++) tab.push_back(phi[p*dpe+a]);
                wphi.push_back(wp);
                for (int a = 0; a+1 < dpe; a++) wphi.push_back(wp*phi[p*dpe+a]);
            }
            npts += npad; nb++;
            (void)st;
        }
        if ((rc = upload(ctx, ctx->b_ttn, tn.data(), tn.size()))) return rc;
        if ((rc = upload(ctx, ctx->b_ttoff, to.data(), to.size()))) return rc;
        if ((rc = upload(ctx, ctx->b_tttab, tab.data(), tab.size()))) return rc;
        if ((rc = upload(ctx, ctx->b_ttwphi, wphi.data(), wphi.size()))) return rc;
        ctx->P.tt_npts = npts;
        // second-generation tile kernels: w, w phi[0..dpe-1] of the packed points (point order of tab)
        std::vector<double> wphif;
        for (int q = 2; q <= qmax && q < 18; q++)
            for (int i = 0; i < tn[q]; i++) {
                const size_t p = (size_t)off[q]+(i < tn[q] ? i : 0);
                const double wp = i < tn[q] ? w[p] : 0.;
                wphif.push_back(wp);
                for (int a = 0; a < dpe; a++) wphif.push_back(wp*phi[p*dpe+a]);
            }
        if ((rc = upload(ctx, ctx->b_ttwphif, wphif.data(), wphif.size()))) return rc;
        if ((rc = upload_uniform_rule_blocks(ctx, qmax, off, bary, w, phi))) return rc;
        ctx->tiles_cached.clear(); ctx->tiles_forms.clear();
    }
    ctx->qmax = qmax;
    ctx->have_rules = true;
    return PNL_OK;
}

int pnl_upload_singular_rule(pnl_context *ctx, int which, int panel, int M, int rows, const double *nodes, const double *w,
                             const double *psi, double facv) {
    if (!ctx) return PNL_ERR_INVALID;
    if (!ctx->have_dofs) return fail(ctx, PNL_ERR_STATE, "upload the DoF map first");
    const int slot = -panel-1;
    const int nslots = which == PNL_INTERIOR ? ctx->dim+1 : ctx->dim;
    if (which < 0 || which > 1 || slot < 0 || slot >= nslots || M <= 0 || rows <= 0 || !nodes || !w || !psi)
        return fail(ctx, PNL_ERR_INVALID, "bad singular-rule arguments");
    const int dim = ctx->dim, dpe = ctx->dpe, dpv = ctx->dpv, dped = ctx->dped, nV = dim+1;
    int rc;
    if (which == PNL_INTERIOR) {
        const int common = slot+1;
        const int expect = common == nV ? dpe : (common == 1 ? 2*dpe-dpv : 2*dpe-2*dpv-dped);
        if (rows != expect) return fail(ctx, PNL_ERR_INVALID, "singular rule has %d rows, expected %d", rows, expect);
        if ((rc = upload(ctx, ctx->C().b_sn[slot], nodes, (size_t)2*nV*M))) return rc;
        if ((rc = upload(ctx, ctx->C().b_sw[slot], w, (size_t)M))) return rc;
        if ((rc = upload(ctx, ctx->C().b_sp[slot], psi, (size_t)rows*M))) return rc;
        ctx->C().sM[slot] = M; ctx->C().sRows[slot] = rows; ctx->C().sFac = facv;
    } else {
        if (rows != dpe) return fail(ctx, PNL_ERR_INVALID, "boundary singular rule has %d rows, expected %d", rows, dpe);
        if ((rc = upload(ctx, ctx->C().b_bn[slot], nodes, (size_t)(nV+dim)*M))) return rc;
        if ((rc = upload(ctx, ctx->C().b_bw[slot], w, (size_t)M))) return rc;
        if ((rc = upload(ctx, ctx->C().b_bp[slot], psi, (size_t)rows*M))) return rc;
        ctx->C().bM[slot] = M; ctx->C().bFac = facv;
    }
    ctx->C().have_sing[which][slot] = true;
    return PNL_OK;
}

int pnl_upload_boundary(pnl_context *ctx, int nb, const int32_t *bcells) {
    if (!ctx) return PNL_ERR_INVALID;
    if (!ctx->have_mesh) return fail(ctx, PNL_ERR_STATE, "upload the mesh first");
    if (nb < 0 || (nb > 0 && !bcells)) return fail(ctx, PNL_ERR_INVALID, "bad boundary arguments");
    ctx->nb = nb;
    ctx->bcells.assign(bcells, bcells+(size_t)nb*ctx->dim);
    ctx->have_boundary = true;
    ctx->dirty = true;
    return PNL_OK;
}

int pnl_tile_cells(pnl_context *ctx) {
    if (!ctx) return PNL_ERR_INVALID;
    int rc = finalize(ctx);
    return rc ? rc : ctx->tile;
}

}  // extern "C"

// ---- tile plan: which tiles a dense assembly visits and which kernel takes each -------------------------------------------
// what the parts of pnl_upload_tiles share
struct TilePlan {
    int T, ncls, L, qlimit, cell_begin, cell_end;
    bool filter, p1, p2, allow, q2ok;
    std::vector<pnl_order_formula> forms;
    std::vector<std::vector<int>> blk_labels;             // variable order: the labels of every block
    std::vector<std::vector<int2>> mixed, uni[3];         // per class: tiles of the general kernel / of one order 2, 3, 4
};

// the option PNL_MIXED_UNSETTLED (a product option, read when the plan is made): the plan settles no mixed tile
static int settled_wanted() { return pnl_tune("PNL_MIXED_UNSETTLED") ? 0 : 1; }
// the option PNL_SETTLED_CODES (a product option, read when the plan is made): the plan keeps the codes of the settled tiles only, and
// the tile kernel builds their pair lists from the codes in every assembly
// Lists are also kept only where the rules of the orders 2, 3 and 4 have 3, 6 and 6 points: the kernel that reads the lists keeps one
// sum per (cell, point) for the diagonal blocks, 3 + 6 + 6 = TileSmem::NR of them (k_tile_distant<.., LISTS>, pnl_kernels.h).
static int lists_wanted(const pnl_context *ctx) {
    if (pnl_tune("PNL_SETTLED_CODES")) return 0;
    for (int q = 2; q <= 4 && q <= ctx->qmax; q++)
        if ((size_t)q+1 >= ctx->rule_off.size() || ctx->rule_off[q+1]-ctx->rule_off[q] != (q == 2 ? 3 : 6)) return 0;
    return 1;
}

// repeated assemblies of the same work list keep it resident
static bool tiles_resident(const pnl_context *ctx, const std::vector<int2> &tiles, const TilePlan &R) {
    const std::vector<pnl_order_formula> &forms = R.forms;
    return tiles.size() == ctx->tiles_cached.size() && ctx->b_tiles.p && ctx->tiles_cb == R.cell_begin && ctx->tiles_ce == R.cell_end &&
        forms.size() == ctx->tiles_forms.size() && std::memcmp(forms.data(), ctx->tiles_forms.data(), sizeof(pnl_order_formula)*R.ncls) == 0 &&
        ctx->tiles_filter == ctx->run.tile_cell_filter && ctx->settled_want == settled_wanted() && ctx->lists_want == lists_wanted(ctx) &&
        (tiles.empty() || std::memcmp(tiles.data(), ctx->tiles_cached.data(), tiles.size()*sizeof(int2)) == 0);
}

// qof[i] for class k: -1 the class does not visit tile i, 2 .. 4 all its pairs are distant pairs of that order, 0 anything else.
// The order bounds of the tiles on a few host threads (4.7 million tiles at 97,537 DoFs), then the exact range on the device.
// open_234: the tiles with qof 0 whose pairs are distant pairs of several of the orders 2 .. 4 (candidates of settle_tiles)
static int tile_orders(pnl_context *ctx, const TilePlan &R, const std::vector<int2> &tiles, int k, std::vector<signed char> &qof,
                       std::vector<size_t> &open_234) {
    open_234.clear();
    const int T = R.T, L = R.L, qlimit = R.qlimit, cell_begin = R.cell_begin, cell_end = R.cell_end;
    const bool filter = R.filter, allow = R.allow, q2ok = R.q2ok;
    const std::vector<std::vector<int>> &blk_labels = R.blk_labels;
    host_threads([&](int th, int nthr) {
        const size_t i0 = tiles.size()*th/nthr, i1 = tiles.size()*(th+1)/nthr;
        for (size_t i = i0; i < i1; i++) {
            const int2 &t = tiles[i];
            bool single = true;
            if (L > 0) {
                bool has = false;
                for (int la : blk_labels[t.x]) for (int lb : blk_labels[t.y])
                    has = has || ctx->cls_of[(size_t)la*L+lb] == k || ctx->cls_of[(size_t)lb*L+la] == k;
                if (!has) { qof[i] = -1; continue; }
                single = blk_labels[t.x].size() == 1 && blk_labels[t.y].size() == 1;
            }
            int q = (allow && single) ? pnl_tile_uniform_order(ctx, R.forms[k], t.x, t.y, qlimit) : 0;
            if (q == 2 && !q2ok) q = 0;
            // the cell range of the MPI-style split applies to the a-cells: only blocks entirely inside qualify
            if (q && filter && !(t.x*T >= cell_begin && (t.x+1)*T <= cell_end)) q = 0;
            qof[i] = (signed char)q;
        }
    });
    // tiles the bounds left open: the exact order range of their cell pairs, on the device (2D; variable order: tiles whose
    // two blocks carry one label each -- their pairs all belong to this class and see its order formula)
    if (!(allow && ctx->dim == 2 && (T == 64 || T == 32))) return PNL_OK;
    std::vector<int2> cand;
    std::vector<size_t> cand_idx;
    for (size_t i = 0; i < tiles.size(); i++) {
        const int2 &t = tiles[i];
        if (qof[i] != 0 || t.x == t.y || !ctx->blocks[t.x].full || !ctx->blocks[t.y].full) continue;
        if (L > 0 && !(blk_labels[t.x].size() == 1 && blk_labels[t.y].size() == 1)) continue;
        if (filter && !(t.x*T >= cell_begin && (t.x+1)*T <= cell_end)) continue;
        cand.push_back(t); cand_idx.push_back(i);
    }
    if (cand.empty()) return PNL_OK;
    int rc;
    if ((rc = upload(ctx, ctx->b_candtiles, cand.data(), cand.size()))) return rc;
    if ((rc = ensure(ctx, ctx->b_candq, cand.size()))) return rc;
    std::vector<signed char> cq(cand.size());
    if ((rc = pnl_tile_order_range(ctx, to_dev(R.forms[k]), (int)cand.size(), cq.data()))) return rc;
    size_t moved = 0;
    for (size_t c = 0; c < cand.size(); c++) {
        const int q = cq[c];
        if (q == -1) open_234.push_back(cand_idx[c]);
        if (q < 2 || q > qlimit || (q == 2 && !q2ok)) continue;
        qof[cand_idx[c]] = (signed char)q; moved++;
    }
    if (pnl_tune("PNL_VERBOSE")) fprintf(stderr, "[pnl] exact order range: %zu of %zu open tiles are uniform\n", moved, cand.size());
    return PNL_OK;
}

// ---- settled tiles (dense 2D P1, one order class without labels, symmetric, the whole cell range) ---------------------------------------
// A mixed tile (a, b), a != b, both blocks full, is settled when the classification of k_tile_distant finds nothing in it but absent
// pairs and distant pairs of the orders 2 .. 4 with a packed rule: most mixed tiles lie in the thin rings where the order steps
// 2 -> 3 -> 4.  That depends on the mesh, the DoF map and the order formula alone -- what this plan is keyed on -- so the plan keeps
// the outcome, 2 bits per pair (k_tile_pair_codes), and the SETTLED instantiation of the tile kernel loads it instead of classifying
// 4096 pairs per tile in every assembly.  k_tile_order_range names the candidates, k_tile_pair_codes decides with the tile kernel's own
// function.  settled: the settled tiles, those with the most pairs of a 6-point rule first (the tile loop hands out tickets: heavy
// tiles first); is_settled: per entry of tiles.  No device memory for the codes, or no packed rules / DoF slots on the device: nothing is
// settled, and that is no error.  The candidates come from the exact order range of tile_orders: where that is skipped (no uniform
// tiles for this element or order table) nothing is settled either.  The code kernel runs twice per plan (statistics of the
// candidates, then the codes of the sorted list): a few milliseconds once per plan against an index array in the hot kernel.
static int settle_tiles(pnl_context *ctx, const TilePlan &R, const std::vector<int2> &tiles, const std::vector<size_t> &open_234,
                        std::vector<int2> &settled, std::vector<char> &is_settled) {
    settled.clear();
    is_settled.assign(tiles.size(), 0);
    if (!settled_wanted() || open_234.empty() || !(R.p1 && ctx->dim == 2 && ctx->dpe == 3 && R.T == 64) || R.ncls != 1 || R.L > 0 ||
        ctx->nonsym || !ctx->b_ttn.p || !ctx->b_cslot.p || R.cell_begin > 0 || R.cell_end < ctx->nc || open_234.size() > (size_t)0x7fffffff/512) return PNL_OK;
    std::vector<int2> cand(open_234.size());
    for (size_t c = 0; c < cand.size(); c++) cand[c] = tiles[open_234[c]];
    int rc;
    if ((rc = upload(ctx, ctx->b_candtiles, cand.data(), cand.size()))) return rc;
    std::vector<int> stat(cand.size());
    if ((rc = pnl_tile_pair_codes(ctx, to_dev(R.forms[0]), (const int2*)ctx->b_candtiles.p, (int)cand.size(), nullptr, stat.data()))) return rc;
    std::vector<size_t> keep;
    for (size_t c = 0; c < cand.size(); c++) if (stat[c] >= 0) keep.push_back(c);
    if (keep.empty()) return PNL_OK;
    if (ensure(ctx, ctx->b_codes, keep.size()*512*sizeof(unsigned short)) != PNL_OK) {
        (void)hipGetLastError();
        ctx->err.clear();
        return PNL_OK;
    }
    std::stable_sort(keep.begin(), keep.end(), [&](size_t x, size_t y) { return stat[x] > stat[y]; });
    for (size_t c : keep) { settled.push_back(cand[c]); is_settled[open_234[c]] = 1; }
    return PNL_OK;
}

// per class: [mixed][order 2][order 3][order 4]
static void tile_lists_per_class(pnl_context *ctx, const TilePlan &R, std::vector<int2> &all) {
    const std::vector<std::vector<int2>> &mixed = R.mixed, *uni = R.uni;
    for (int k = 0; k < R.ncls; k++) {
        ctx->cls_tile_off[k] = (int)all.size(); ctx->cls_n_mixed[k] = (int)mixed[k].size();
        all.insert(all.end(), mixed[k].begin(), mixed[k].end());
        for (int u = 0; u < 3; u++) { ctx->cls_n_uni[u][k] = (int)uni[u][k].size(); all.insert(all.end(), uni[u][k].begin(), uni[u][k].end()); }
        ctx->cls_n_pure[k] = ctx->cls_n_uni[0][k];
    }
}

// one launch over all classes: [mixed tiles of all classes][order 2][order 3][order 4]; class word = 2 class + orientation
// (a non-symmetric order table visits every mixed tile once per orientation)
static int tile_lists_single_launch(pnl_context *ctx, const TilePlan &R, const std::vector<int2> &tiles, std::vector<int2> &all) {
    const int ncls = R.ncls;
    const std::vector<std::vector<int2>> &mixed = R.mixed, *uni = R.uni;
    std::vector<int32_t> allcls;
    const int norient = ctx->nonsym ? 2 : 1;
    ctx->sl_off[0] = 0;
    // symmetric order tables: a tile that holds pairs of several classes gets ONE entry that names the set of them (bit 29
    // + class bits); k_tile_p2 works through the classes inside one visit and flushes once with plain stores
    const bool one_visit = norient == 1 && ncls > 1 && ncls <= 28;
    std::vector<unsigned> tile_mask;
    if (one_visit) {
        tile_mask.assign((size_t)ctx->nblocks*ctx->nblocks, 0u);
        for (int k = 0; k < ncls; k++)
            for (const int2 &t : mixed[k]) tile_mask[(size_t)t.x*ctx->nblocks+t.y] |= 1u << k;
        // the multi-class tiles first (several classifications each: the heavy ones), in tile-list order
        for (const int2 &t : tiles) {
            const unsigned m = tile_mask[(size_t)t.x*ctx->nblocks+t.y];
            if (m & (m-1u)) { all.push_back(t); allcls.push_back((int)((1u << 29) | m)); }
        }
    }
    for (int k = 0; k < ncls; k++) {
        ctx->cls_n_mixed[k] = (int)mixed[k].size();
        for (int o = 0; o < norient; o++)
            for (const int2 &t : mixed[k]) {
                if (one_visit) { const unsigned m = tile_mask[(size_t)t.x*ctx->nblocks+t.y]; if (m & (m-1u)) continue; }
                all.push_back(t); allcls.push_back(2*k+o);
            }
    }
    ctx->sl_n[0] = (int)all.size();
    for (int u = 0; u < 3; u++) {
        ctx->sl_off[u+1] = (int)all.size();
        for (int k = 0; k < ncls; k++) {
            ctx->cls_n_uni[u][k] = (int)uni[u][k].size();
            for (const int2 &t : uni[u][k]) { all.push_back(t); allcls.push_back(2*k); }
        }
        ctx->sl_n[u+1] = (int)all.size()-ctx->sl_off[u+1];
    }
    for (int k = 0; k < ncls; k++) ctx->cls_n_pure[k] = ctx->cls_n_uni[0][k];
    // tiles that are visited more than once (several classes, both orientations) add into the block-slot storage
    // (bit 30 of the class word) and are zeroed before
    std::vector<long long> keys(all.size());
    for (size_t i = 0; i < all.size(); i++) keys[i] = (long long)all[i].x*ctx->nblocks+all[i].y;
    std::vector<long long> sorted(keys);
    std::sort(sorted.begin(), sorted.end());
    std::vector<int2> multi;
    for (size_t i = 0; i+1 < sorted.size(); i++)
        if (sorted[i] == sorted[i+1] && (i == 0 || sorted[i-1] != sorted[i]))
            multi.push_back(make_int2((int)(sorted[i]/ctx->nblocks), (int)(sorted[i]%ctx->nblocks)));
    std::vector<long long> mk(multi.size());
    for (size_t i = 0; i < multi.size(); i++) mk[i] = (long long)multi[i].x*ctx->nblocks+multi[i].y;
    for (size_t i = 0; i < all.size(); i++)
        if (std::binary_search(mk.begin(), mk.end(), keys[i])) allcls[i] |= (1 << 30);
    ctx->n_multitiles = (int)multi.size();
    int rc;
    if ((rc = upload(ctx, ctx->b_multitiles, multi.data(), multi.size()))) return rc;
    return upload(ctx, ctx->b_tilecls, allcls.data(), allcls.size());
}

int pnl_upload_tiles(pnl_context *ctx, std::vector<int2> &tiles, int cell_begin, int cell_end) {
    TilePlan R;
    const int ncls = R.ncls = (int)ctx->cls.size();
    R.cell_begin = cell_begin; R.cell_end = cell_end;
    R.forms = std::vector<pnl_order_formula>(ncls);
    for (int k = 0; k < ncls; k++) R.forms[k] = ctx->cls[k]->form[0];
    if (tiles_resident(ctx, tiles, R)) return PNL_OK;
    const int T = R.T = ctx->tile;
    R.filter = ctx->run.tile_cell_filter;
    // uniform tiles: order 2 through k_tile_pure (P1 in 1D and 2D), orders 2-4 through k_tile_uniform (2D: P1 orders 3 and 4, P2)
    R.p1 = T == 64 && (ctx->dpe == 3 || ctx->dpe == 2); R.p2 = ctx->dim == 2 && ctx->dpe == 6;
    R.allow = (R.p1 || R.p2) && ctx->qmax >= 2 && !ctx->nonsym;
    int qlimit = 2;
    if (ctx->dim == 2) for (int q = 3; q <= 4 && ctx->uni_off[q] >= 0 && ctx->uni_np[q] == 6 && q <= ctx->qmax; q++) qlimit = q;
    R.q2ok = R.p1 ? true : (ctx->uni_off[2] >= 0 && ctx->uni_np[2] == 3);
    R.qlimit = qlimit;
    // variable order: a class only visits the tiles whose blocks hold a label pair of that class (most blocks carry one
    // label, so the K passes together classify every tile about once instead of K times)
    const int L = R.L = ctx->nlab;
    std::vector<std::vector<int>> &blk_labels = R.blk_labels;
    if (L > 0) {
        blk_labels.resize(ctx->nblocks);
        for (int b = 0; b < ctx->nblocks; b++) {
            auto &v = blk_labels[b];
            for (int c = b*T; c < std::min((b+1)*T, ctx->nc); c++) v.push_back(ctx->cell_labels[c]);
            std::sort(v.begin(), v.end());
            v.erase(std::unique(v.begin(), v.end()), v.end());
        }
    }
    ctx->cls_tile_off.assign(ncls, 0); ctx->cls_n_mixed.assign(ncls, 0); ctx->cls_n_pure.assign(ncls, 0);
    for (int u = 0; u < 3; u++) ctx->cls_n_uni[u].assign(ncls, 0);
    std::vector<std::vector<int2>> &mixed = R.mixed, *uni = R.uni;
    mixed.resize(ncls);
    for (int u = 0; u < 3; u++) uni[u].resize(ncls);
    // the lists in tile order
    std::vector<signed char> qof(tiles.size());
    std::vector<size_t> open_234;
    std::vector<int2> settled;
    std::vector<char> is_settled;
    int rc;
    ctx->n_settled = 0;
    for (int k = 0; k < ncls; k++) {
        if ((rc = tile_orders(ctx, R, tiles, k, qof, open_234))) return rc;
        if ((rc = settle_tiles(ctx, R, tiles, open_234, settled, is_settled))) return rc;
        for (size_t i = 0; i < tiles.size(); i++) {
            const int q = qof[i];
            if (q < 0 || is_settled[i]) continue;
            (q ? uni[q-2][k] : mixed[k]).push_back(tiles[i]);
        }
        // the mixed list: its unsettled part in tile order (heavy first), then the settled tiles
        mixed[k].insert(mixed[k].end(), settled.begin(), settled.end());
    }
    if (settled.empty()) ctx->b_codes.release();
    if (settled.empty() || !lists_wanted(ctx)) ctx->b_lists.release();
    ctx->settled_tiles.clear();
    std::vector<int2> all;
    ctx->single_launch = R.p2;
    if (!R.p2) tile_lists_per_class(ctx, R, all);
    else if ((rc = tile_lists_single_launch(ctx, R, tiles, all))) return rc;
    if (pnl_tune("PNL_VERBOSE")) {
        size_t nm = 0, nu[3] = {0, 0, 0};
        for (int k = 0; k < ncls; k++) { nm += mixed[k].size(); for (int u = 0; u < 3; u++) nu[u] += uni[u][k].size(); }
        fprintf(stderr, "[pnl] tiles: %zu mixed (%zu of them settled), uniform order 2/3/4: %zu / %zu / %zu (qlimit %d)\n", nm, settled.size(),
                nu[0], nu[1], nu[2], qlimit);
    }
    if ((rc = upload(ctx, ctx->b_tiles, all.data(), all.size()))) return rc;
    if (!settled.empty()) {
        // the pair codes in the order of the list (settled implies one class: its mixed tiles are the first entries of b_tiles)
        const int first = ctx->cls_tile_off[0]+ctx->cls_n_mixed[0]-(int)settled.size();
        if ((rc = pnl_tile_pair_codes(ctx, to_dev(R.forms[0]), (const int2*)ctx->b_tiles.p+first, (int)settled.size(),
                                      (unsigned short*)ctx->b_codes.p, nullptr))) return rc;
        ctx->n_settled = (int)settled.size();
        ctx->settled_tiles = settled;
        ctx->code_builds++;
        // the pair lists of these codes.  No device memory for them: the settled tiles stay settled and are taken by their codes
        if (lists_wanted(ctx)) {
            if (ensure(ctx, ctx->b_lists, settled.size()*PNL_LIST_STRIDE*sizeof(unsigned short)) != PNL_OK) {
                (void)hipGetLastError();
                ctx->err.clear();
                ctx->b_lists.release();
            } else if ((rc = pnl_tile_pair_lists(ctx, (const unsigned short*)ctx->b_codes.p, (int)settled.size(), (unsigned short*)ctx->b_lists.p)))
                return rc;
        }
    }
    ctx->settled_want = settled_wanted();
    ctx->lists_want = lists_wanted(ctx);
    ctx->tiles_cached = tiles; ctx->tiles_cb = cell_begin; ctx->tiles_ce = cell_end; ctx->tiles_forms = R.forms;
    ctx->tiles_filter = ctx->run.tile_cell_filter;
    return PNL_OK;
}

int pnl_make_tiles(pnl_context *ctx, std::vector<int2> &tiles, int cell_begin, int cell_end) {
    const int T = ctx->tile, nbk = ctx->nblocks;
    const int a0 = cell_begin/T, a1 = (cell_end+T-1)/T;
    // heavy (near-diagonal) tiles first
    for (int d = 0; d < nbk; d++)
        for (int a = a0; a < a1 && a+d < nbk; a++) tiles.push_back(make_int2(a, a+d));
    return PNL_OK;
}

extern "C" {

// Estimated cost of every block row of the upper block triangle, in units of one uniform order-2 tile: what a rank that owns
// the row spends on its tiles (classified like upload_tiles does, weights from the measured time per tile of the kernels:
// profiles/r02b_*) plus the per-cell work of its cells (touching pairs, boundary term).
int pnl_block_row_costs(pnl_context *ctx, double *out, int n) {
    if (!ctx || !out) return PNL_ERR_INVALID;
    int rc;
    if ((rc = check_ready(ctx))) return rc;
    if ((rc = finalize(ctx))) return rc;
    if (n != ctx->nblocks) return fail(ctx, PNL_ERR_INVALID, "pnl_block_row_costs: %d blocks expected", ctx->nblocks);
    const int T = ctx->tile, nb = ctx->nblocks;
    const bool p1 = T == 64 && (ctx->dpe == 3 || ctx->dpe == 2), p2 = ctx->dim == 2 && ctx->dpe == 6;
    const bool allow = (p1 || p2) && ctx->qmax >= 2 && !ctx->nonsym && ctx->cls.size() == 1;
    int qlimit = 2;
    if (ctx->dim == 2) for (int q = 3; q <= 4 && ctx->uni_off[q] >= 0 && ctx->uni_np[q] == 6 && q <= ctx->qmax; q++) qlimit = q;
    const pnl_order_formula F = ctx->cls[0]->form[0];
    // ns per tile at 98,304 cells (P1: 51 / 138 / 204 incl. its work-list pairs) and 24,576 cells (P2: 50 / 87 / 125)
    const double w_uni3 = p2 ? 1.75 : 2.7, w_mixed = p2 ? 2.5 : 4.0, w_cells = p2 ? 30. : 57.;
    host_threads([&](int t, int nthreads) {
        for (int a = t; a < nb; a += nthreads) {
            double c = w_cells;
            for (int b = a; b < nb; b++) {
                const int q = allow ? pnl_tile_uniform_order(ctx, F, a, b, qlimit) : 0;
                c += q == 2 ? 1. : (q ? w_uni3 : w_mixed);
            }
            out[a] = c;
        }
    });
    return PNL_OK;
}

// ---- non-symmetric kernels with an order s(x) per quadrature point ------------------------------------------------------
int pnl_set_order_function(pnl_context *ctx, const pnl_order_function *f, const double *cell_smax, const double *facet_smax,
                           double c0, double bc0, double sing_fac, double bsing_fac) {
    if (!ctx || !f || !cell_smax) return fail(ctx, PNL_ERR_INVALID, "bad order-function arguments");
    if (!ctx->have_mesh) return fail(ctx, PNL_ERR_STATE, "upload the mesh first");
    if (f->type < 1 || f->type > 5) return fail(ctx, PNL_ERR_UNSUPPORTED, "order function type %d is not implemented", f->type);
    if (ctx->have_dofs && !(ctx->dpe == ctx->dim+1 || (ctx->dim == 2 && ctx->dpe == 6) || (ctx->dim == 1 && ctx->dpe == 3)))
        return fail(ctx, PNL_ERR_UNSUPPORTED, "pointwise variable orders: P1 and P2 elements");
    if (!pw_set_function(ctx->pw, *f)) return fail(ctx, PNL_ERR_INVALID, "bad Chebyshev series of the scaling");
    ctx->pw.c0 = c0; ctx->pw.bc0 = bc0; ctx->pw.sfac = sing_fac; ctx->pw.bfac = bsing_fac;
    ctx->pw_cell_smax.assign(cell_smax, cell_smax+ctx->nc);
    ctx->pw_facet_smax.clear();
    if (facet_smax && ctx->have_boundary) ctx->pw_facet_smax.assign(facet_smax, facet_smax+ctx->nb);
    for (int w = 0; w < 2; w++) for (int s = 0; s < 3; s++) ctx->have_pw_rules[w][s] = false;
    ctx->pw_vertex_s.clear();
    ctx->have_pw = true;
    return PNL_OK;
}

int pnl_set_order_vertex_values(pnl_context *ctx, int nv, const double *values) {
    if (!ctx || !values) return PNL_ERR_INVALID;
    if (!ctx->have_pw || ctx->pw.type != 5) return fail(ctx, PNL_ERR_STATE, "set an order function of type 5 first");
    if (nv != ctx->nv) return fail(ctx, PNL_ERR_INVALID, "pnl_set_order_vertex_values: %d vertices expected", ctx->nv);
    ctx->pw_vertex_s.assign(values, values+nv);
    return PNL_OK;
}

int pnl_upload_pointwise_rules(pnl_context *ctx, int which, int panel, int nkeys, int M, int rows, const double *nodes,
                               const double *w, const double *phi0, const double *phi1) {
    if (!ctx) return PNL_ERR_INVALID;
    if (!ctx->have_pw || !ctx->have_dofs) return fail(ctx, PNL_ERR_STATE, "set the order function and the DoF map first");
    const int slot = -panel-1, dim = ctx->dim, nV = dim+1, dpe = ctx->dpe;
    const int nslots = which == PNL_INTERIOR ? nV : dim;
    if (which < 0 || which > 1 || slot < 0 || slot >= nslots || nkeys <= 0 || M <= 0 || !nodes || !w || !phi0 ||
        (which == PNL_INTERIOR && !phi1))
        return fail(ctx, PNL_ERR_INVALID, "bad pointwise-rule arguments");
    int rc;
    if (which == PNL_INTERIOR) {
        const int common = slot+1;
        const int expect = common == nV ? dpe : (common == 1 ? 2*dpe-ctx->dpv : 2*dpe-2*ctx->dpv-ctx->dped);
        if (rows != expect) return fail(ctx, PNL_ERR_INVALID, "pointwise rule has %d rows, expected %d", rows, expect);
        if ((rc = upload(ctx, ctx->b_pw_rule[0][slot][0], nodes, (size_t)nkeys*2*nV*M))) return rc;
        if ((rc = upload(ctx, ctx->b_pw_rule[0][slot][1], w, (size_t)nkeys*M))) return rc;
        if ((rc = upload(ctx, ctx->b_pw_rule[0][slot][2], phi0, (size_t)nkeys*rows*M))) return rc;
        if ((rc = upload(ctx, ctx->b_pw_rule[0][slot][3], phi1, (size_t)nkeys*rows*M))) return rc;
        ctx->pw.M[slot] = M; ctx->pw.rows[slot] = rows;
        ctx->pw.nodes[slot] = (const double*)ctx->b_pw_rule[0][slot][0].p; ctx->pw.w[slot] = (const double*)ctx->b_pw_rule[0][slot][1].p;
        ctx->pw.phi0[slot] = (const double*)ctx->b_pw_rule[0][slot][2].p; ctx->pw.phi1[slot] = (const double*)ctx->b_pw_rule[0][slot][3].p;
    } else {
        if (rows != dpe) return fail(ctx, PNL_ERR_INVALID, "pointwise boundary rule has %d rows, expected %d", rows, dpe);
        if ((rc = upload(ctx, ctx->b_pw_rule[1][slot][0], nodes, (size_t)nkeys*(nV+dim)*M))) return rc;
        if ((rc = upload(ctx, ctx->b_pw_rule[1][slot][1], w, (size_t)nkeys*M))) return rc;
        if ((rc = upload(ctx, ctx->b_pw_rule[1][slot][2], phi0, (size_t)nkeys*rows*M))) return rc;
        ctx->pw.bM[slot] = M;
        ctx->pw.bnodes[slot] = (const double*)ctx->b_pw_rule[1][slot][0].p; ctx->pw.bw[slot] = (const double*)ctx->b_pw_rule[1][slot][1].p;
        ctx->pw.bphi[slot] = (const double*)ctx->b_pw_rule[1][slot][2].p;
    }
    ctx->pw_nkeys[which] = nkeys;
    ctx->have_pw_rules[which][slot] = true;
    return PNL_OK;
}

}  // extern "C"

// what every assembly with an order per quadrature point needs before its first launch (the entry points are in
// pnl_pwnear.hip; nothing is launched here): padded cell tables, the per-cell / per-facet largest orders and the vertex values of
// a P1 order function on the device, the distant rules in the problem description
int pnl_pw_prepare(pnl_context *ctx, int need_boundary) {
    int rc;
    if (!ctx->have_pw || !ctx->have_rules) return fail(ctx, PNL_ERR_STATE, "order function and distant rules must be set before assembling");
    if ((rc = finalize(ctx))) return rc;
    if (ctx->pw.type == 5) {
        if ((int)ctx->pw_vertex_s.size() != ctx->nv) return fail(ctx, PNL_ERR_STATE, "order function of type 5 without vertex values");
        const int nV = ctx->dim+1;
        std::vector<double> sv((size_t)nV*ctx->ncp, 0.);
        for (int c = 0; c < ctx->nc; c++)
            for (int k = 0; k < nV; k++) sv[(size_t)k*ctx->ncp+c] = ctx->pw_vertex_s[ctx->cells[(size_t)c*nV+k]];
        if ((rc = upload(ctx, ctx->b_pw_cellsv, sv.data(), sv.size()))) return rc;
        ctx->pw.cell_sv = (const double*)ctx->b_pw_cellsv.p; ctx->pw.sv_stride = ctx->ncp;
    }
    if (!(ctx->dpe == ctx->dim+1 || (ctx->dim == 2 && ctx->dpe == 6) || (ctx->dim == 1 && ctx->dpe == 3)))
        return fail(ctx, PNL_ERR_UNSUPPORTED, "pointwise variable orders: P1 and P2 elements");
    for (int s = 0; s <= ctx->dim; s++)
        if (!ctx->have_pw_rules[0][s]) return fail(ctx, PNL_ERR_STATE, "pointwise rule for %d common vertices not uploaded", s+1);
    if (need_boundary) {
        if (!ctx->have_boundary || (int)ctx->pw_facet_smax.size() != ctx->nb)
            return fail(ctx, PNL_ERR_STATE, "the boundary term needs boundary facets and their orders");
        for (int s = 0; s < ctx->dim; s++)
            if (!ctx->have_pw_rules[1][s]) return fail(ctx, PNL_ERR_STATE, "pointwise boundary rule for %d common vertices not uploaded", s+1);
    }
    std::vector<double> sm(ctx->ncp, 0.);
    std::copy(ctx->pw_cell_smax.begin(), ctx->pw_cell_smax.end(), sm.begin());
    if ((rc = upload(ctx, ctx->b_pw_csm, sm.data(), sm.size()))) return rc;
    if ((rc = upload(ctx, ctx->b_pw_fsm, ctx->pw_facet_smax.data(), ctx->pw_facet_smax.size()))) return rc;
    ctx->pw.cell_smax = (const double*)ctx->b_pw_csm.p; ctx->pw.facet_smax = (const double*)ctx->b_pw_fsm.p;
    DevProblem &P = ctx->P;
    P.qmax = ctx->qmax;
    P.off = (const int*)ctx->b_off.p; P.bary = (const double*)ctx->b_bary.p; P.w = (const double*)ctx->b_w.p;
    P.phi = (const double*)ctx->b_phi.p; P.foff = (const int*)ctx->b_foff.p; P.fbary = (const double*)ctx->b_fbary.p;
    P.fw = (const double*)ctx->b_fw.p;
    P.cur_class = -1;
    return PNL_OK;
}

extern "C" {

int pnl_get_counters(pnl_context *ctx, int64_t *out, int n) {
    if (!ctx || !out || n <= 0) return PNL_ERR_INVALID;
    if (!ctx->b_counters.p) return fail(ctx, PNL_ERR_STATE, "nothing assembled yet");
    unsigned long long tmp[PNL_NCOUNTERS];
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    HIPCHK(ctx, hipMemcpy(tmp, ctx->b_counters.p, sizeof(tmp), hipMemcpyDeviceToHost));
    tmp[0] = ctx->run.visited_is_assembled ? tmp[1] : ctx->run.visited_pairs;
    for (int i = 0; i < n && i < PNL_C_SETTLED_TILES; i++) out[i] = (int64_t)tmp[i];
    if (n > PNL_C_UNIFORM_TILES_UNCHECKED) out[PNL_C_UNIFORM_TILES_UNCHECKED] = (int64_t)tmp[PNL_DC_UNI_TILES_UNCHECKED];
    if (n > PNL_C_UNIFORM_TILES_CHECKED) out[PNL_C_UNIFORM_TILES_CHECKED] = (int64_t)tmp[PNL_DC_UNI_TILES_CHECKED];
    if (n > PNL_C_SETTLED_TILES) out[PNL_C_SETTLED_TILES] = ctx->run.settled_run;
    if (n > PNL_C_SETTLED_LIST_TILES) out[PNL_C_SETTLED_LIST_TILES] = ctx->run.lists_run;
    if (n > PNL_C_CODE_BUILDS) out[PNL_C_CODE_BUILDS] = ctx->code_builds;
    if (n > PNL_C_WORKLIST_LENGTH) {
        // entries the tile kernels handed to the work lists, over the passes of the assembly (the fill counters check_overflow reads)
        unsigned wl[PNL_WL_SLOTS];
        const int ns = std::min(ctx->run.wl_slots, PNL_WL_SLOTS);
        out[PNL_C_WORKLIST_LENGTH] = 0;
        if (ctx->b_wlcount.p && ctx->wl_cap_each > 0) {
            HIPCHK(ctx, hipMemcpy(wl, ctx->b_wlcount.p, sizeof(unsigned)*std::max(1, ns), hipMemcpyDeviceToHost));
            for (int i = 0; i < ns; i++) out[PNL_C_WORKLIST_LENGTH] += wl[i];
        }
    }
    return check_overflow(ctx);
}

int pnl_get_phase_ms(pnl_context *ctx, float *out, int n) {
    if (!ctx || !out || n <= 0) return PNL_ERR_INVALID;
    if (!ctx->run.ev_valid) return fail(ctx, PNL_ERR_STATE, "nothing assembled yet");
    HIPCHK(ctx, hipEventSynchronize(ctx->ev[EV_END]));
    float t[7] = {0, 0, 0, 0, 0, 0, 0}, tmp;
    if (ctx->run.tiles_launched) {
        HIPCHK(ctx, hipEventElapsedTime(&t[0], ctx->ev[EV_START], ctx->ev[EV_TILES_DONE]));           // tile kernels (uniform + general; last class)
        HIPCHK(ctx, hipEventElapsedTime(&t[1], ctx->ev[EV_TILES_DONE], ctx->ev[EV_WORKLIST_DONE]));   // work-list kernels
        if (ctx->run.pure_launched && ctx->cls.size() == 1) {
            HIPCHK(ctx, hipEventElapsedTime(&t[6], ctx->ev[EV_START], ctx->ev[EV_TILES_UNIFORM_DONE]));   // uniform-tile kernel alone
            t[0] -= t[6];
        }
    }
    HIPCHK(ctx, hipEventElapsedTime(&tmp, ctx->ev[EV_WORKLIST_DONE], ctx->ev[EV_MIRROR_DONE]));       // mirror
    HIPCHK(ctx, hipEventElapsedTime(&t[2], ctx->ev[EV_MIRROR_DONE], ctx->ev[EV_SINGULAR_DONE]));      // singular
    HIPCHK(ctx, hipEventElapsedTime(&t[3], ctx->ev[EV_SINGULAR_DONE], ctx->ev[EV_BOUNDARY_DONE]));      // boundary
    HIPCHK(ctx, hipEventElapsedTime(&t[4], ctx->ev[EV_BOUNDARY_DONE], ctx->ev[EV_END]));      // diagonal scatter
    t[4] += tmp;
    HIPCHK(ctx, hipEventElapsedTime(&t[5], ctx->ev[EV_START], ctx->ev[EV_END]));
    for (int i = 0; i < n && i < 7; i++) out[i] = t[i];
    return PNL_OK;
}

int pnl_get_settled_tiles(pnl_context *ctx, int32_t *tiles, int64_t ntiles) {
    if (!ctx || ntiles < 0 || (ntiles && !tiles)) return PNL_ERR_INVALID;
    if (!ctx->b_tiles.p || ctx->cls_n_mixed.empty()) return fail(ctx, PNL_ERR_STATE, "no tile plan yet");
    const std::vector<int2> &st = ctx->settled_tiles;
    if ((int)st.size() != ctx->n_settled) return fail(ctx, PNL_ERR_STATE, "the resident tile list is not that of a dense assembly");
    for (size_t i = 0; i < st.size() && (int64_t)i < ntiles; i++) { tiles[2*i] = st[i].x; tiles[2*i+1] = st[i].y; }
    return (int)st.size();
}

int pnl_get_settled_lists(pnl_context *ctx, uint16_t *codes, uint16_t *lists, int64_t ntiles) {
    if (!ctx || ntiles < 0) return PNL_ERR_INVALID;
    if (!ctx->b_tiles.p || ctx->cls_n_mixed.empty()) return fail(ctx, PNL_ERR_STATE, "no tile plan yet");
    const int64_t n = std::min<int64_t>(ntiles, ctx->n_settled);
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (codes && n > 0) HIPCHK(ctx, hipMemcpy(codes, ctx->b_codes.p, (size_t)n*512*sizeof(uint16_t), hipMemcpyDeviceToHost));
    if (lists && n > 0) {
        if (!ctx->b_lists.p) return fail(ctx, PNL_ERR_STATE, "the resident tile plan keeps no pair lists");
        HIPCHK(ctx, hipMemcpy(lists, ctx->b_lists.p, (size_t)n*PNL_LIST_STRIDE*sizeof(uint16_t), hipMemcpyDeviceToHost));
    }
    return ctx->b_lists.p ? ctx->n_settled : 0;
}

int pnl_uniform_lane_layout(int nc, const int32_t *cells, const int32_t *dofs, int mode, int nthreads, int32_t *sizes, uint8_t *lane_cell,
                            int16_t *lds_col, int8_t *vorder, int16_t *cell_col, double *mult, double *seconds) {
    if (nc <= 0 || !cells || !dofs || !sizes || mode < 0 || mode > 2) return PNL_ERR_INVALID;
    const int T = 64, nblocks = (nc+T-1)/T, ncp = nblocks*T;
    // unique DoFs per block and the slots of the cells, as finalize() makes them
    std::vector<int16_t> cslot((size_t)3*ncp, -1);
    std::vector<std::vector<int>> lists(nblocks);
    int nU = 1;
    for (int b = 0; b < nblocks; b++) {
        auto &L = lists[b];
        for (int c = b*T; c < std::min(nc, (b+1)*T); c++) for (int k = 0; k < 3; k++) if (dofs[(size_t)c*3+k] >= 0) L.push_back(dofs[(size_t)c*3+k]);
        std::sort(L.begin(), L.end());
        L.erase(std::unique(L.begin(), L.end()), L.end());
        nU = std::max<int>(nU, (int)L.size());
    }
    sizes[0] = nblocks; sizes[1] = nU; sizes[2] = mode == 0 ? 0 : 16*uni_lane_cap(nU)+16; sizes[3] = ncp;
    if (!lane_cell || !lds_col || !vorder || !cell_col || !mult) return PNL_OK;
    std::vector<int> cl(cells, cells+(size_t)nc*3), lperm((size_t)nc*3);
    for (int c = 0; c < nc; c++) for (int k = 0; k < 3; k++) lperm[(size_t)c*3+k] = k;
    host_threads([&](int th, int nthr) {
        for (int b = th; b < nblocks; b += nthr) tile_order_block(b, nc, T, cl.data(), lperm.data());
    }, nthreads);
    for (int c = 0; c < nc; c++)
        for (int k = 0; k < 3; k++) {
            const int g = dofs[(size_t)c*3+lperm[(size_t)c*3+k]];
            const auto &L = lists[c/T];
            if (g >= 0) cslot[(size_t)k*ncp+c] = (int16_t)(std::lower_bound(L.begin(), L.end(), g)-L.begin());
        }
    const auto t0 = std::chrono::steady_clock::now();
    UniLaneTables tabs[3];
    uni_lane_layout(nblocks, ncp, nU, cslot.data(), tabs, nthreads);
    if (seconds) *seconds = std::chrono::duration<double>(std::chrono::steady_clock::now()-t0).count();
    const UniLaneTables &R = tabs[mode];
    std::copy(R.lane_cell.begin(), R.lane_cell.end(), lane_cell);
    std::copy(R.lds_col.begin(), R.lds_col.end(), lds_col);
    std::copy(R.cell_col.begin(), R.cell_col.end(), cell_col);
    std::copy(R.mult.begin(), R.mult.end(), mult);
    for (size_t i = 0; i < lperm.size(); i++) vorder[i] = (int8_t)lperm[i];
    return PNL_OK;
}

int pnl_get_kernel_ms(pnl_context *ctx, float *out, int n) {
    if (!ctx || !out || n <= 0) return PNL_ERR_INVALID;
    if (!ctx->run.ev_valid) return fail(ctx, PNL_ERR_STATE, "nothing assembled yet");
    HIPCHK(ctx, hipEventSynchronize(ctx->ev[EV_END]));
    for (int s = 0; s < n && s < PNL_NUM_KERNEL_SLOTS; s++) {
        out[s] = 0.f;
        for (int k = 0; k < ctx->run.kev_n[s]; k++) {
            float t = 0.f;
            HIPCHK(ctx, hipEventElapsedTime(&t, ctx->kev[s][2*k], ctx->kev[s][2*k+1]));
            out[s] += t;
        }
    }
    return PNL_OK;
}

}  // extern "C"
