// Internal: the context behind the C ABI (include/pnl_hip.h), shared by the translation units of libpnl_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "pnl_hip.h"
#include "pnl_device.h"

constexpr int TILE_P1 = 64;     // cells per block for dpe <= 3
constexpr int TILE_P2 = 32;     // cells per block for dpe == 6 (bigger LDS sub-block per cell)

struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    ~DevBuf() { release(); }
    void release() { if (p) { (void)hipFree(p); p = nullptr; bytes = 0; } }
};

// The phase events of an assembly (pnl_context::ev).  Every assembly path records all of them on the caller's stream, in the order
// START, TILES_UNIFORM_DONE, TILES_DONE, WORKLIST_DONE, MIRROR_DONE, SINGULAR_DONE, BOUNDARY_DONE, END; a path without a phase records
// its event right behind the one before.  pnl_get_phase_ms reads the differences.  EV_TILES_DONE and EV_TILES_UNIFORM_DONE are also
// events that side streams wait for (the boundary term beside the fold pass).  The values are the slots of the array.
enum PhaseEvent {
    EV_START = 0,               // counters and diagonal-block buffer zeroed, nothing launched yet
    EV_WORKLIST_DONE = 1,       // work-list kernels (behind the fold + mirror pass of a block-slot assembly)
    EV_MIRROR_DONE = 2,         // k_mirror of an assembly without block-slot storage
    EV_SINGULAR_DONE = 3,       // touching pairs (joined, where they ran on a side stream)
    EV_BOUNDARY_DONE = 4,       // boundary term joined
    EV_END = 5,                 // diagonal blocks scattered
    EV_TILES_DONE = 6,          // last tile kernel (of the last class pass)
    EV_TILES_UNIFORM_DONE = 7,  // uniform tiles
    EV_COUNT = 8
};

// What one assembly leaves for its own later phases and for pnl_get_counters / pnl_get_phase_ms / pnl_get_kernel_ms, and what means
// nothing for the next assembly.  pnl_begin_assembly starts every C-ABI assembly call with a fresh record; each path then sets only
// what it knows.  Plan state that survives assemblies (tile lists, n_settled, wl_cap ...) stays in the context.
struct AssemblyRun {
    bool ev_valid = false;          // the phase events are all recorded: false until the assembly has succeeded
    bool tiles_launched = false, pure_launched = false;     // phases "tiles" / "tiles_uniform" of pnl_get_phase_ms exist
    bool symflush = false;          // PNL_FLAG_SYMMETRIC_FLUSH
    bool tile_cell_filter = true;   // apply [cell_begin, cell_end) to the a-cells of the tiles too (not for a caller's tile list)
    bool full_tile_list = false;    // the tile list is the whole upper block triangle of the cell range (pnl_assemble_dense)
    // the tile kernels wrote the block-slot storage; ev_fold is recorded behind a fold + mirror pass
    bool slot_used = false, fold_event_set = false;
    int settled_run = 0;            // tiles taken through k_tile_distant<.., SETTLED>
    int lists_run = 0;              // ... of them through k_tile_distant<.., SETTLED, LISTS> (pair lists of the plan)
    int tile_off = 0, n_mixed = 0, n_pure = 0;      // slice of b_tiles of the class pass being launched (dense P1 / 1D)
    // fill counters of b_wlcount in use (one per class / pass; 0: the path keeps none): pnl_get_counters sums them, check_overflow
    int wl_slots = 0;               // holds them against wl_cap_each
    int uni_ctr_next = 0, uni_ctr_fresh = 0;        // ticket counters of b_unictr: next to hand out, how many are still zeroed
    int kev_n[PNL_NUM_KERNEL_SLOTS] = {}; bool kev_open[PNL_NUM_KERNEL_SLOTS] = {};    // timed launches per kernel slot (pairs of pnl_context::kev in use)
    unsigned long long visited_pairs = 0;   // numCellPairs of pnl_get_counters, unless
    bool visited_is_assembled = false;      // (finite-horizon tiles) every visited (non-REMOTE) pair is an assembled one
};

// host copy of the lane layout tables (UniLanes, pnl_device.h)
struct UniLaneTables {
    std::vector<unsigned char> lane_cell;
    std::vector<short> lds_col, cell_col;       // cell_col in cell order [3][ncp] (pnl_uni_lanes_ready permutes the device copy)
    std::vector<double> mult;         // [nblocks] modelled LDS cycles of a sub-block add over the conflict-free ones
    int stride = 0;                   // row stride of the sub-block in doubles (0: the launcher's rule for the identity layout)
};

struct pnl_context {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    // side streams for the per-class passes of a variable order (work list, touching pairs, boundary): the passes only add
    // to A / the diagonal blocks with atomics, so they may overlap; each fills the other's tail (ClassFork in pnl_hip.hip)
    static constexpr int NAUX = 4;      // side streams (the runtime maps streams onto four hardware queues: more streams share them; measured, no gain from six)
    hipStream_t aux[NAUX] = {};
    hipEvent_t ev_fork = nullptr, ev_join[NAUX] = {};
    // recorded behind the fold + mirror pass of a block-slot assembly: from here on A only receives atomic adds, so the touching
    // pairs and the boundary term run on side streams next to the work-list kernels (one order class)
    hipEvent_t ev_fold = nullptr;
    std::string err;
    // host copies
    int dim = 0, nv = 0, nc = 0, dpe = 0, dpv = 0, dped = 0, N = 0, nb = 0, qmax = -1;
    int nreal = 0;                            // cells of positive volume (the others are in-mesh padding, finalize())
    std::vector<int> cell_orig;               // the caller's number of every cell (pnl_set_cell_order), empty = the numbering of the upload
    std::vector<int> real_from;               // [nc + 1] number of real cells with index >= c
    double H0 = 0.;
    std::vector<double> vertices, vol, h;
    std::vector<int32_t> cells, dofs, perm_table, bcells;
    // per order class (one class for a constant order; pnl_set_classes for a piecewise-constant variable order): kernel,
    // order formula, singular rules and the touching pairs that belong to the class
    struct ClassData {
        pnl_kernel kern[2];
        pnl_order_formula form[2];
        bool have_kernel[2] = {false, false}, have_form[2] = {false, false};
        bool have_sing[2][3] = {{false, false, false}, {false, false, false}};
        DevBuf b_sn[3], b_sw[3], b_sp[3], b_bn[2], b_bw[2], b_bp[2], b_spairs[3], b_bpairs[2], b_spairs1[3];
        int sM[3] = {0, 0, 0}, sRows[3] = {0, 0, 0}, bM[2] = {0, 0};
        double sFac = 0., bFac = 0.;
        int n_spairs[3] = {0, 0, 0}, n_bpairs[2] = {0, 0};
        int n_spairs1[3] = {0, 0, 0};   // non-symmetric order: touching pairs (c2, c1) of the second orientation
        ClassData() { std::memset(kern, 0, sizeof(kern)); std::memset(form, 0, sizeof(form)); }
    };
    std::vector<ClassData*> cls;
    int cur = 0;                      // class the setters and launchers currently act on
    ClassData &C() { return *cls[cur]; }
    int nlab = 0;                     // labels of the variable order (0: constant order)
    bool nonsym = false;              // cls_of is not symmetric: both orientations of every pair (pnl_set_nonsymmetric)
    int orient = 0;                   // orientation the launchers currently act on
    std::vector<int32_t> cell_labels, facet_labels, cls_of;
    bool have_mesh = false, have_dofs = false, have_rules = false, have_boundary = false;
    bool dirty = true;
    // device
    DevProblem P;
    DevBuf b_cellv, b_ccen, b_cvol, b_ch, b_clog, b_cvid, b_cdof, b_cslot, b_blk_ndof, b_blk_dofs, b_perm, b_off, b_bary, b_w, b_phi,
        b_foff, b_fbary, b_fw, b_bvid, b_bv, b_bgeo, b_counters, b_D, b_tiles,
        b_vec[6], b_clabel, b_blabel, b_clsof, b_scal, b_wl, b_wlcount, b_tilectr, b_ttn, b_ttoff, b_tttab, b_ttwphi, b_wlsorted, b_wlaux,
        b_vertices, b_sp_indptr, b_sp_indices, b_mp_pairs, b_mp_masks, b_mp_wl, b_mp_sorted, b_mp_aux, b_bi_cells, b_bi_facets,
        b_bi_masks, b_cp[28], b_cpD, b_wlds, b_wlpair, b_h2[27];
    // second-generation tile kernels (pnl_tile2.h): per-class kernel / order-formula tables, rules of the uniform-order tiles,
    // class word of every tile entry (2 class + orientation), w and w phi of the packed rules
    DevBuf b_kcls, b_fcls, b_uni, b_tilecls, b_ttwphif;
    // block-slot storage (pnl_tile2.h): padded column offsets of the blocks, row offsets, copies (block, slot) of every DoF,
    // the tiles that several order classes visit, the storage itself (allocated by the first assembly that uses it)
    DevBuf b_scolbase, b_srowoff, b_cpoff, b_cpslot, b_cprow, b_foldtab, b_bkcls, b_bfcls, b_bdefer, b_multitiles, b_slotA, b_candtiles, b_candq;
    int slot_S = 0, n_multitiles = 0;
    // settled tiles of the resident plan (dense 2D P1, one order class; pnl_setup.hip: settle_tiles): the last n_settled mixed tiles of
    // b_tiles, their pair codes in b_codes (512 16-bit words per tile, allocated with the tile lists and dropped with them).
    // settled_want: the plan was made without the option PNL_MIXED_UNSETTLED; code_builds: times this context has computed codes
    // b_lists: the pair lists of the settled tiles, derived from the codes (one record of PNL_LIST_STRIDE 16-bit words per tile,
    // pnl_device.h; k_tile_distant<.., SETTLED, LISTS> reads them instead of building the lists from the codes in every assembly).  Empty with the
    // option PNL_SETTLED_CODES or where the device has no memory for them: the assembly then takes the settled tiles by their codes.
    // lists_want: the plan was made without PNL_SETTLED_CODES
    DevBuf b_codes, b_lists;
    int n_settled = 0, settled_want = -1, lists_want = -1;
    std::vector<int2> settled_tiles;              // host copy of the settled part of the list (pnl_get_settled_tiles)
    long long code_builds = 0;
    // ticket counters of the uniform-tile launches (b_unictr, UNI_CTRS words): an assembly zeroes all of them at its start and hands
    // them out in turn (AssemblyRun::uni_ctr_fresh left); launches beyond that zero their counter in the stream themselves
    DevBuf b_unictr;
    static constexpr int UNI_CTRS = 64;
    long long slot_total = 0;         // doubles
    // row slab of a rank (pnl_set_row_slab, pnl_slab.hip)
    DevBuf b_rowmap, b_rowdof, b_colmap, b_coldof;
    DevBuf b_cholinfo;                // pnl_potrf (pnl_direct.hip): the word that takes the first pivot that is not positive
    DevBuf b_luwork, b_lutmp;         // pnl_getrf (pnl_direct.hip): info word, ticket, pivot rows, partial maxima; pnl_getrs: the permuted right-hand sides
    DevBuf b_blk_part, b_blk_xt;      // pnl_block.hip: partial sums of the column chunks [chunk][16][nrows]; the transposed group of vectors [n][NV]
    DevBuf b_kb_part;                 // pnl_krylov_block.h: partial sums of the dot products of the block Krylov steps [5][256][16]
    DevBuf b_cgb_work, b_bcgb_work;   // pnl_cg_jacobi_block: dinv, R, P, AP, Z and the state; pnl_bicgstab_block: dinv, seven blocks and the state
    DevBuf b_eigb_part;               // pnl_eig_block.hip: the partial tiles of pnl_eigb_gram [workgroup][9 tile pairs][16 x 16]
    std::vector<int32_t> slab_rowdofs, slab_coldofs;
    int slab_rows = 0, slab_cols = 0;
    std::vector<DevKernel> kcls_host;
    std::vector<DevKernel> bkcls_host;
    std::vector<DevFormula> bfcls_host;
    std::vector<DevFormula> fcls_host;
    int uni_off[5] = {-1, -1, -1, -1, -1}, uni_np[5] = {0, 0, 0, 0, 0};
    // the 3-point rule of P1 has equal weights and shape values w phi_b(y_j) = A + B delta_bj (points reordered to make it so):
    // k_tile_uniform<3, 3, KT, true> forms the cross block from row, column and total sums of the nine kernel values
    bool uni_struct[5] = {false, false, false, false, false};
    H2Dev h2;
    bool have_h2 = false;
    // non-symmetric kernels with an order per quadrature point (pnl_set_order_function)
    bool have_tile_order = false;     // permuted cell tables for the tile kernels (finalize starts the search, tile_order_ready ends it)
    struct TileOrderJob *tile_job = nullptr;
    DevBuf b_cellv_t, b_cdof_t, b_cslot_t, b_Dt;    // b_Dt: diagonal blocks in the tile kernels' local order
    // 2D P1: lane layout of the blocks for k_tile_uniform (pnl_setup.hip: uni_lane_layout), one set of tables per value of the option
    // PNL_UNI_LANES (0 identity, 1 searched, 2 random); the device copies hold the set uni_lanes_up (-1: none)
    UniLaneTables uni_lanes[3];
    int uni_lanes_up = -1;
    double uni_lanes_seconds = 0.;
    DevBuf b_ul_cell, b_ul_col, b_ul_ccol, b_ul_cellv, b_ul_cvol, b_ul_cslot, b_ul_real;
    std::vector<double> ul_cellv_t;             // host copies of the cell tables in the tile kernels' vertex order, for the lane-ordered
    std::vector<short> ul_cslot_t;              // device tables of a layout
    PwDev pw;
    bool have_pw = false, have_pw_rules[2][3] = {{false, false, false}, {false, false, false}};
    int pw_nkeys[2] = {0, 0};
    std::vector<double> pw_cell_smax, pw_facet_smax;
    std::vector<double> pw_vertex_s;           // order function of type 5: values at the mesh vertices
    DevBuf b_pw_cellsv;
    DevBuf b_pw_csm, b_pw_fsm, b_pw_rule[2][3][4], b_pw_pairs, b_pw_bpairs;
    std::vector<std::vector<int>> h2_levels;   // nodes of every level >= 1
    long long h2_vtot = 0;                    // doubles of the leaf values V (pnl_h2_get / _set)
    std::vector<size_t> h2_level_off;
    // block far field (pnl_h2_block.hip): b_h2[20 .. 24] = pairs per n1 (ptr, idx), children per node (ptr, idx), parents by level
    // with h2_par_off [nlevels + 1] into that list; b_h2[25], [26] = the context's own cupB / cdownB [nnodes][M][16]
    std::vector<size_t> h2_par_off;
    std::vector<int32_t> rule_off, frule_off;   // host copies of the distant-rule offsets (cell points, facet points) per order
    int sp_nnz = -1;                // near-field sparsity pattern (pnl_upload_sparsity)
    unsigned wl_cap = 0;
    int tile = TILE_P1, nblocks = 0, ncp = 0, nU = 0;
    std::vector<int2> spairs_host[3];
    std::vector<int2> tiles_cached;   // tile list (as given by the caller) currently resident in b_tiles
    size_t tiles_cap = 0;
    // b_tiles holds the mixed tiles first, then the uniform ones (all pairs distant with the lowest order)
    int tiles_cb = -1, tiles_ce = -1;
    std::vector<int> cls_tile_off, cls_n_mixed, cls_n_pure;     // per order class: its slice of b_tiles (mixed tiles, then uniform)
    std::vector<int> cls_n_uni[3];    // uniform tiles of order 2, 3, 4 per class (cls_n_pure = cls_n_uni[0]); they follow the mixed ones
    // dim 2, dpe 6 (one launch over all classes): b_tiles = [mixed tiles of all classes][order 2][order 3][order 4], b_tilecls alike
    bool single_launch = false;
    int sl_off[4] = {0, 0, 0, 0}, sl_n[4] = {0, 0, 0, 0};
    unsigned wl_cap_each = 0;         // capacity of one work-list region (one region per class in a single-launch assembly)
    std::vector<pnl_order_formula> tiles_forms;
    pnl_order_formula tiles_form;
    bool tiles_filter = true;
    // tables of the general power (pnl_pow_tab, pnl_common.h), one per (exponent, scale) seen by this context
    struct PowTab { double exponent, scale; DevBuf buf; };
    std::vector<PowTab*> powtabs;
    // tcx / tcy / trad: centre and radius (cell centres + vertex reach) in the coordinates of the interaction transform
    struct BlockAgg { double cx, cy, rad, hmax, hmin, Lmin, Lmax; bool full; double tcx, tcy, trad; };
    // linear transform of the interaction set (ellipse domains, interactionDomains.pyx:1393-1630): the kernel sees |T (x - y)|
    bool have_xform = false;
    double xform[4] = {1., 0., 0., 1.};
    std::vector<BlockAgg> blocks;
    hipEvent_t ev[EV_COUNT] = {};     // the phase events, by PhaseEvent
    // event pair around every tile-kernel launch (pnl_get_kernel_ms); a slot that is launched several times per assembly (the
    // order classes) takes one more pair per launch, created on first use and kept; AssemblyRun::kev_n counts the launches
    std::vector<hipEvent_t> kev[PNL_NUM_KERNEL_SLOTS];
    AssemblyRun run;                // the assembly in progress or, behind it, the last one (pnl_begin_assembly)
};

// once per C-ABI assembly call, where its arguments have been checked and before anything of the run is set
inline void pnl_begin_assembly(pnl_context *ctx) { ctx->run = AssemblyRun{}; }

inline int fail(pnl_context *ctx, int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf;
    return code;
}

#define HIPCHK(ctx, call)                                                                            \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess) return fail(ctx, PNL_ERR_HIP, "%s failed: %s", #call, hipGetErrorString(e_)); \
    } while (0)

template <class T>
int upload(pnl_context *ctx, DevBuf &b, const T *src, size_t n) {
    const size_t bytes = std::max<size_t>(n*sizeof(T), 16);
    if (b.bytes < bytes) {
        b.release();
        HIPCHK(ctx, hipMalloc(&b.p, bytes));
        b.bytes = bytes;
    }
    if (n) HIPCHK(ctx, hipMemcpyAsync(b.p, src, n*sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    // host vectors passed here may be temporaries: make the copy synchronous
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PNL_OK;
}

inline int ensure(pnl_context *ctx, DevBuf &b, size_t bytes) {
    bytes = std::max<size_t>(bytes, 16);
    if (b.bytes < bytes) {
        b.release();
        HIPCHK(ctx, hipMalloc(&b.p, bytes));
        b.bytes = bytes;
    }
    return PNL_OK;
}

inline DevKernel to_dev(const pnl_kernel &k, int dim) {
    DevKernel d;
    d.ktype = k.ktype;
    d.exponent = k.exponent;
    d.scale = k.scale;
    d.horizon2 = k.horizon2;
    d.interaction = k.interaction;
    // quarter-integer exponents get the rsqrt-based evaluation
    const double m4 = -4.*k.exponent;
    const int qm = (int)std::lround(m4);
    (void)dim;
    d.qm = qm;
    d.fast = (k.ktype == PNL_FRACTIONAL && std::isinf(k.horizon2) && qm >= 1 && qm <= 32 && std::fabs(m4-qm) < 1e-13) ? 1 : 0;
    {
        long double b = 1.L;
        for (int i = 0; i < 6; i++) { b *= ((long double)k.exponent-i)/(long double)(i+1); d.pb[i] = (double)b; }
    }
    d.ptab = nullptr;
    return d;
}

// the boundary kernel as the boundary tiles evaluate it (DevProblem::bkn): in 2D the 1/|x-y| of the normal factor n.(y-x)/|y-x|
// folded into the exponent of a fractional kernel, the folded 2D forms 7 / 8 of the Gauss-theorem twins (kern_eval, pnl_common.h)
inline DevKernel to_dev_bkn(pnl_kernel kn, int dim) {
    if (dim == 2 && kn.ktype == PNL_FRACTIONAL) kn.exponent -= 0.5;
    DevKernel d = to_dev(kn, dim);
    if (dim == 2 && kn.ktype != PNL_FRACTIONAL) d.fast = 0;
    if (dim == 2 && kn.ktype == PNL_GAUSSIAN_BOUNDARY) d.ktype = 7;
    if (dim == 2 && kn.ktype == PNL_EXPONENTIAL_BOUNDARY) d.ktype = 8;
    return d;
}

// values of the pnl_pow_tab tables of k (PNL_POW_TAB_DOUBLES doubles, scale folded in; pnl_setup.hip); false where the kernel
// has none (not fractional, or fast without also_fast, or the option PNL_NO_POWTAB)
bool pow_table_values(const DevKernel &k, bool also_fast, std::vector<double> &tab);
// pnl_setup.hip: the same tables on the device, one copy per (exponent, scale) of the context; nullptr where there are none
const double *pnl_pow_table(pnl_context *ctx, const DevKernel &k, bool also_fast = false);

// the order function's part of PwDev (the rest is per mesh: pnl_set_order_function); false: a bad Chebyshev series of the scaling
inline bool pw_set_function(PwDev &W, const pnl_order_function &f) {
    std::memset(&W, 0, sizeof(W));
    W.type = f.type; W.normalized = f.normalized;
    for (int i = 0; i < 6; i++) W.p[i] = f.p[i];
    if (f.scal_n < 0 || f.scal_n > 32 || (f.scal_n > 0 && !(f.scal_half > 0.))) return false;
    W.scal_n = f.scal_n; W.scal_mid = f.scal_mid; W.scal_inv_half = f.scal_n > 0 ? 1./f.scal_half : 0.;
    for (int i = 0; i < 32; i++) W.scal_cheb[i] = i < f.scal_n ? f.scal_cheb[i] : 0.;
    return true;
}

inline DevFormula to_dev(const pnl_order_formula &f) {
    DevFormula d;
    d.c0 = f.c0; d.a = f.a; d.b = f.b; d.e = f.e; d.den0 = f.den0; d.clip = f.clip_num; d.pad = 0;
    return d;
}

// Options of the library.  It reads NO environment variable on the assembly path: an option exists only after
// pnl_set_option(name, value) named it, and pnl_set_option accepts the names of k_product_options (pnl_setup.hip; listed in
// include/pnl_hip.h) only -- the hooks the parity tests use to reach the alternative code paths, and the diagnostics.  Call it with
// a literal name: tests/test_abi.py holds the call sites against that table.  Returns the value string or nullptr.
const char *pnl_tune(const char *name);
// grid of a persistent tile kernel, capped by the option PNL_TILE_WGS (tests)
inline int pnl_grid_cap(int grid) {
    const char *e = pnl_tune("PNL_TILE_WGS");
    const int cap = e ? atoi(e) : 0;
    return cap > 0 ? std::max(1, std::min(grid, cap)) : grid;
}

// row stride of the LDS sub-block: nU + 1 columns (+1: trash column / row for boundary DoFs), rounded up to 1 mod 32 doubles:
// rows that start in different LDS banks see fewer conflicts in the ds_add_f64 of the cross blocks (measured: -0.4 ms at
// noRef 6), if the bigger sub-block still leaves two workgroups per CU
inline int acc_stride_of(int nU, size_t fixed_bytes = 0) {
    constexpr int m = 32;
    int st = nU+1, padded = st;
    while (padded % m != 1) padded++;
    if (fixed_bytes+sizeof(double)*(size_t)(nU+1)*padded <= 80*1024) st = padded;
    else if (st % 2 == 0 && fixed_bytes+sizeof(double)*(size_t)(nU+1)*(st+1) <= 80*1024) st++;    // at least an odd stride
    return st;
}

// the problem description the dense tile kernels see: cell tables in the conflict-reducing local vertex order
inline DevProblem tile_problem(const pnl_context *ctx) {
    DevProblem Pt = ctx->P;
    if (ctx->have_tile_order) {
        Pt.cellv = (const double*)ctx->b_cellv_t.p; Pt.cdof = (const int*)ctx->b_cdof_t.p; Pt.cslot = (const short*)ctx->b_cslot_t.p;
    }
    return Pt;
}

// what the mixed-tile kernel (k_tile_distant) needs beyond that: the orbit-ordered rule blocks of the orders 2 .. 4 and the orders
// whose pairs take the structured evaluators (2D P1, rules with the orbit structure; none with the option PNL_MIXED_GENERIC)
inline DevProblem with_mixed_rules(const pnl_context *ctx, DevProblem Pt) {
    Pt.uni = (const double*)ctx->b_uni.p;
    Pt.mix_struct = 0;
    const bool generic = pnl_tune("PNL_MIXED_GENERIC") != nullptr;
    for (int q = 0; q < 5; q++) {
        Pt.uni_off[q] = ctx->uni_off[q] >= 0 ? ctx->uni_off[q] : 0;
        if (q >= 2 && q <= ctx->qmax && ctx->dim == 2 && ctx->dpe == 3 && ctx->uni_off[q] >= 0 && ctx->uni_struct[q] && !generic)
            Pt.mix_struct |= 1 << q;
    }
    return Pt;
}

inline void kt_begin(pnl_context *ctx, int slot) {
    std::vector<hipEvent_t> &v = ctx->kev[slot];
    const size_t k = 2*(size_t)ctx->run.kev_n[slot];
    ctx->run.kev_open[slot] = false;
    while (v.size() < k+2) {
        hipEvent_t e = nullptr;
        if (hipEventCreate(&e) != hipSuccess) { (void)hipGetLastError(); return; }      // no timer for this launch
        v.push_back(e);
    }
    ctx->run.kev_open[slot] = hipEventRecord(v[k], ctx->stream) == hipSuccess;
}
inline void kt_end(pnl_context *ctx, int slot) {
    if (!ctx->run.kev_open[slot]) return;
    ctx->run.kev_open[slot] = false;
    if (hipEventRecord(ctx->kev[slot][2*(size_t)ctx->run.kev_n[slot]+1], ctx->stream) == hipSuccess) ctx->run.kev_n[slot]++;
}

// pnl_setup.hip: joins the vertex-order search finalize() started and uploads the permuted cell tables (sets have_tile_order)
int pnl_tile_order_ready(pnl_context *ctx);
// pnl_setup.hip: the lane layout tables of the option PNL_UNI_LANES on the device (2D P1, after pnl_tile_order_ready); *mode: the value
// in force, *stride: row stride of the LDS sub-block in doubles (0: the launcher's own rule, mode 0)
int pnl_uni_lanes_ready(pnl_context *ctx, UniLanes *UL, int *mode, int *stride);

// pnl_setup.hip: what pnl_h2_setup (pnl_h2.hip) shares with the assemblies of a constant or piecewise constant order -- kernels, order
// formulas and rules are set, the tables derived from mesh and DoF map exist (finalize), the problem description holds the current class
int pnl_assembly_prepare(pnl_context *ctx);
// its two halves: the checks with finalize; the problem description of the class / orientation ctx->cur / ctx->orient (launches nothing)
int pnl_assembly_ready(pnl_context *ctx);
void pnl_refresh_tables(pnl_context *ctx);

// ctx->stream, ctx->cur and ctx->orient are implicit arguments of every launcher.  They change through these two scopes only, which put
// them back on every way out of the region.
// The launchers inside the scope go to `stream` (to() switches again); afterwards ctx->stream is what it was before
struct StreamScope {
    pnl_context *ctx;
    hipStream_t prev;
    StreamScope(pnl_context *c, hipStream_t stream) : ctx(c), prev(c->stream) { ctx->stream = stream; }
    StreamScope(const StreamScope&) = delete; StreamScope &operator=(const StreamScope&) = delete;
    void to(hipStream_t stream) { ctx->stream = stream; }
    ~StreamScope() { ctx->stream = prev; }
};
// select(k, orient): setters and launchers act on order class k in that orientation, ctx->P describes it.  Afterwards the class is
// leave_at and the orientation 0: the dense and the cluster assemblies leave class 0, the CSR pair assemblies the class they were
// entered with (the caller's pnl_select_class holds).  refresh_after: ctx->P describes that class again
struct ClassScope {
    pnl_context *ctx;
    int leave_at;
    bool refresh_after;
    ClassScope(pnl_context *c, int leave_at_, bool refresh_after_ = false) : ctx(c), leave_at(leave_at_), refresh_after(refresh_after_) {}
    ClassScope(const ClassScope&) = delete; ClassScope &operator=(const ClassScope&) = delete;
    void select(int k, int orient) { ctx->cur = k; ctx->orient = orient; pnl_refresh_tables(ctx); }
    ~ClassScope() { ctx->cur = leave_at; ctx->orient = 0; if (refresh_after) pnl_refresh_tables(ctx); }
};
// pnl_setup.hip, the tile plan of a dense assembly: the tiles (block a, block b >= a) of a cell range, heavy ones first; which of
// the caller's tiles are of one order, the lists per class / of the single-launch P2 layout in b_tiles (kept while nothing changes)
int pnl_make_tiles(pnl_context *ctx, std::vector<int2> &tiles, int cell_begin, int cell_end);
int pnl_upload_tiles(pnl_context *ctx, std::vector<int2> &tiles, int cell_begin, int cell_end);
// pnl_hip.hip, for pnl_upload_tiles: k_tile_order_range<ctx->tile> over the ncand tiles in b_candtiles, one order (or 0) each into
// host_out through b_candq; synchronises the stream
int pnl_tile_order_range(pnl_context *ctx, const DevFormula &qo, int ncand, signed char *host_out);
// pnl_hip.hip, for pnl_upload_tiles: k_tile_pair_codes over n tiles of 64 cells (device pointer): codes (device, 512 words per tile) and /
// or host_stat (per tile -1 not settled, else its number of pairs of a 6-point rule) may be nullptr; synchronises the stream
int pnl_tile_pair_codes(pnl_context *ctx, const DevFormula &qo, const int2 *tiles, int n, unsigned short *codes, int *host_stat);
// pnl_hip.hip, for pnl_upload_tiles: k_tile_pair_lists, the list records (device, PNL_LIST_STRIDE words per tile) of n settled tiles from
// their codes (device); synchronises the stream
int pnl_tile_pair_lists(pnl_context *ctx, const unsigned short *codes, int n, unsigned short *lists);
// pnl_hip.hip: counting sort of a work list by order (k_wl_hist / _scan / _scatter): histogram, offsets, 16-pair chunk offsets and cursors
// of the bins, PNL_WL_BINS + 1 words each, carved out of aux_base
struct WlBins { unsigned *hist, *offs, *coff, *cursor; };
int pnl_wl_sort(pnl_context *ctx, const int4 *wl, const unsigned *count, unsigned cap, unsigned *aux_base, int4 *sorted, WlBins &B);
// pnl_hip.hip: the per-cell diagonal blocks D into the dense matrix (k_scatter_diag<ctx->dpe>, dpe 2, 3 or 6)
void pnl_scatter_diag(pnl_context *ctx, const DevProblem &P, const double *D, double *A, int64_t ldA);
// pnl_setup.hip: the one order <= qlimit of all cell pairs of the tile (block ta, block tb), 0 where that cannot be proved
int pnl_tile_uniform_order(const pnl_context *ctx, const pnl_order_formula &F, int ta, int tb, int qlimit);
// pnl_sparse.hip: pnl_assembly_ready, the uploaded pattern and the output checked, pnl_refresh_tables, S filled in -- in that order
int pnl_sparse_ready(pnl_context *ctx, double *data, double *diag, SparseOut &S);

// pnl_h2_block.hip, for pnl_h2_setup once it has validated the plan: the index structures of the block far field
int pnl_h2_block_plan(pnl_context *ctx, const pnl_h2_plan *pl);

// pnl_setup.hip / pnl_pwnear.hip: kernels with an order per quadrature point
int pnl_pw_prepare(pnl_context *ctx, int need_boundary);
int pnl_pw_h2_interp(pnl_context *ctx);

// pnl_gemv2.hip: one pass over a row-major block for both A x and A^T x
int pnl_launch_gemv_symmetric(pnl_context *ctx, const double *A, long long ldA, int n, const double *x, double alpha, double beta,
                              const double *b, double *y);
int pnl_launch_slab_two_sided(pnl_context *ctx, const double *slab, long long ld, int nrows, int ncols, const int *rowdof, const int *coldof,
                              const double *x, double *y);

// pnl_tile2.hip
int pnl2_launch_uniform(pnl_context *ctx, int kt, const DevProblem &Pt, const int2 *tiles, const int *tile_cls, int ntiles, int q,
                        double *A, int64_t ldA, double *Dglob, const SlotOut &SO);
int pnl2_launch_p2(pnl_context *ctx, int kt, const int2 *tiles, const int *tile_cls, int ntiles, double *A, int64_t ldA,
                   int cell_begin, int cell_end, unsigned wl_cap_each, const SlotOut &SO);
int pnl2_zero_slot_tiles(pnl_context *ctx, const SlotOut &SO);
int pnl2_fold_mirror(pnl_context *ctx, const SlotOut &SO, double *A, int64_t ldA);
inline SlotOut slot_out(const pnl_context *ctx) {
    SlotOut SO;
    SO.A2 = (double*)ctx->b_slotA.p; SO.rowoff = (const long long*)ctx->b_srowoff.p; SO.colbase = (const int*)ctx->b_scolbase.p;
    SO.S = ctx->slot_S; SO.nU = ctx->nU;
    return SO;
}
