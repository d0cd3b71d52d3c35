/* pnl_hip.h -- C ABI of the MI355X (gfx950) nonlocal-assembly library libpnl_hip.so.
 *
 * This is the drop-in boundary for the hot path of PyNucleus_nl's nonlocalBuilder:
 * the double loop over element pairs that classifies the pair, integrates the
 * kernel over it and scatters the local matrix (reference, Cython, CPU only):
 *
 *   nl/PyNucleus_nl/nonlocalAssembly_{SCALAR}.pxi:1262-1473   nonlocalBuilder.getDense
 *   nl/PyNucleus_nl/nonlocalOperator_decl_{SCALAR}.pxi:8-91   the cdef seam it sits behind
 *        (setMesh1/2, setCell1/2, getPanelType(), eval(contrib, panel, mask))
 *   nl/PyNucleus_nl/kernelsCy.pxd:17                          kernel_fun_t(x, y, c_params)
 *
 * The reference has no C ABI of its own; every entry point below names the
 * reference routine(s) whose work it takes over.  Plain pointers and sizes only --
 * no Python, numpy or torch types.  Pointers named *_host are read on the CPU and
 * copied into HBM by the library; pointers named *_dev must be device memory
 * (hipMalloc / a torch.cuda tensor's data_ptr).  All indices are int32, all reals
 * fp64, arrays are C-contiguous (the reference's INDEX_t / REAL_t, myTypes64.pxd).
 *
 * Error convention: every function returns 0 on success or a negative pnl_status;
 * pnl_error_string() returns a description of the last failure of that context.
 * The host layer maps PNL_ERR_UNSUPPORTED to NotImplementedError and
 * PNL_ERR_INVALID to AssertionError like the reference (NA:915, 941, 1022, 1055).
 * A context is single-caller like the reference's builder objects; internally
 * every call is asynchronous on the context's HIP stream unless stated otherwise.
 */
#ifndef PNL_HIP_H
#define PNL_HIP_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pnl_context pnl_context;

enum pnl_status {
    PNL_OK = 0,
    PNL_ERR_INVALID = -1,       /* bad argument / inconsistent sizes           */
    PNL_ERR_UNSUPPORTED = -2,   /* (dim, element, kernel) combination not built */
    PNL_ERR_HIP = -3,           /* a HIP runtime call failed                    */
    PNL_ERR_STATE = -4,         /* called before the required uploads           */
    PNL_ERR_ORDER = -5          /* a pair needs a quadrature order beyond the uploaded tables */
};

/* PNL_GAUSSIAN: scale exp(exponent |x-y|^2), exponent = -1/(horizon/3)^2 or -1/(2 variance^dim) (kernelsCy.pyx:388-416, 687-692);
 * PNL_EXPONENTIAL: scale exp(exponent |x-y|), exponent = -rate (kernelsCy.pyx:448-462);
 * PNL_GAUSSIAN_BOUNDARY / PNL_EXPONENTIAL_BOUNDARY: their Gauss-theorem twins on the full space, to be set as the boundary kernel
 * (kernelsCy.pyx:418-477): 1D scale sqrt(pi / -exponent) erfc(sqrt(-exponent) |x-y|), 2D scale exp(exponent |x-y|^2) / (-exponent |x-y|);
 * 2 scale exp(exponent |x-y|) / -exponent */
enum pnl_kernel_type { PNL_FRACTIONAL = 0, PNL_INDICATOR = 1, PNL_PERIDYNAMIC = 2, PNL_GAUSSIAN = 3, PNL_EXPONENTIAL = 4,
                       PNL_GAUSSIAN_BOUNDARY = 5, PNL_EXPONENTIAL_BOUNDARY = 6 };

/* gamma(x,y) = scale * (|x-y|^2)^exponent inside |x-y|^2 <= horizon2 (inf: everywhere).
 * Replaces the opaque c_kernel_params block + kernelFun pointer (kernel_params.pxi:8-30,
 * kernelsCy.pyx:75-294).  interaction (finite horizon only): how element pairs cut by the horizon are integrated,
 * 1 = ball2_retriangulation (interactionDomains.pyx:395-822, 866-980), 2 = ball2_barycenter (:340-392, 982-1067).
 * Finite-horizon kernels are assembled from an explicit pair list (pnl_assemble_pairs_masked = getSparse NA:1062-1260). */
typedef struct {
    int32_t ktype;
    int32_t interaction;
    double exponent;
    double scale;
    double horizon2;
} pnl_kernel;

/* Distant-pair quadrature order (fractionalLaplacian2D.pyx:622-642, :1226-1243,
 * fractionalLaplacian1D.pyx:234-253, :646-660):
 * order = max(ceil((c0 + a*L_other + b*Lmax - e*logdh_other)/(max(logdh_self,0)+den0)), 2) */
typedef struct {
    double c0, a, b, e, den0;
    int32_t clip_num;
    int32_t pad;
} pnl_order_formula;

#define PNL_INTERIOR 0
#define PNL_BOUNDARY 1

/* counters (pnl_get_counters), names after the reference's PLogger values NA:1834-1838 */
enum pnl_counter {
    PNL_C_NUM_CELL_PAIRS = 0,          /* pairs visited (c1 <= c2)                       */
    PNL_C_NUM_ASSEMBLED_CELL_PAIRS,    /* pairs with panel != IGNORED                    */
    PNL_C_NUM_INTEGRATIONS,            /* kernel evaluations, interior                   */
    PNL_C_NUM_BOUNDARY_PAIRS,
    PNL_C_NUM_BOUNDARY_INTEGRATIONS,
    PNL_C_ORDER_OVERFLOW,              /* pairs whose order exceeded the tables (error)  */
    PNL_C_UNIFORM_TILE_PAIRS,          /* pairs integrated by the uniform-tile kernel (subset of assembled) */
    PNL_C_RESERVED7,
    PNL_C_HIST0 = 8,                   /* [8+q]: distant pairs of order q, q < 120; [128..130]: vertex/edge/face */
    PNL_C_UNIFORM_Q2 = 131,            /* [131..133]: pairs integrated by the uniform-tile kernels of order 2, 3, 4 */
    PNL_C_SETTLED_TILES = 134,         /* mixed tiles the assembly took through the settled instantiation of the tile kernel  */
    PNL_C_CODE_BUILDS = 135,           /* times the context has computed the pair codes of settled tiles (once per tile plan)  */
    PNL_C_WORKLIST_LENGTH = 136,       /* entries the tile kernels handed to the device work lists, summed over the passes      */
    PNL_C_SETTLED_LIST_TILES = 137,    /* settled tiles the assembly took with the pair lists of the plan (the others: by their codes) */
    PNL_C_UNIFORM_TILES_UNCHECKED = 138, /* P1 uniform tiles whose cells are all real and have a DoF: pair loop without the validity test */
    PNL_C_UNIFORM_TILES_CHECKED = 139  /* P1 uniform tiles taken through the pair loop that tests every pair (all with PNL_UNI_CHECKED) */
};
#define PNL_NUM_COUNTERS 140

/* Options (process-wide).  The library reads no environment variable on its assembly path; an option exists once it has been
 * set here (value NULL removes it).  The library accepts
 *   "PNL_WL_FRAC"     capacity of the device work lists as a fraction of the candidate pairs (tests force the overflow report),
 *   "PNL_FH_NOTILES"  finite horizon: every pair through the per-pair pipeline instead of the block tiles,
 *   "PNL_NO_POWTAB"   general exponent: exp(e ln x) instead of the table-driven power,
 *   "PNL_BND_OLD"     Omega x Omega^c term: the per-pair kernel instead of the tiled one (2D),
 *   "PNL_PLAN_THREADS" host threads of the planner,
 *   "PNL_TILE_WGS"    at most this many workgroups per persistent tile kernel (tests: every workgroup then walks many tiles),
 *   "PNL_UNI_GENERIC" uniform-order tiles: the evaluator for arbitrary rules also where the rule has the orbit structure of the
 *                     symmetric 3- and 6-point rules (tests: both evaluators against each other),
 *   "PNL_UNI_CHECKED" P1 uniform-order tiles: every tile through the pair loop that tests whether a pair exists, also the tiles whose
 *                     cells are all real and have a DoF (tests: both loops against each other; read at every launch),
 *   "PNL_UNI_LANES"   P1 uniform-order tiles: the lane layout of the blocks (pnl_uniform_lane_layout) -- 1 searched (the default), 0 lane =
 *                     cell and column = slot with the row stride 1 mod 32 (the access pattern before the layout existed), 2 random
 *                     (tests: results do not rest on the layout; read at every launch),
 *   "PNL_MIXED_GENERIC" mixed tiles: the evaluators for arbitrary rules also for the pairs whose rule has that orbit structure
 *                     (tests: both evaluators against each other),
 *   "PNL_MIXED_UNSETTLED" the tile plan settles no mixed tile: every mixed tile is classified pair by pair in every assembly
 *                     (tests: both paths against each other; read when the plan is made, changing it makes a new plan),
 *   "PNL_SETTLED_CODES" the tile plan keeps the pair codes of the settled tiles but not their pair lists: the tile kernel builds the lists
 *                     of a settled tile from its codes in every assembly (tests and A/B measurement; read when the plan is made,
 *                     changing it makes a new plan).  The plan does the same by itself where the device has no memory for the lists,
 *   "PNL_NO_OVERLAP", "PNL_NO_FORK"   profiling: no side streams, every phase on the caller's stream one after the other,
 *   "PNL_VERBOSE", "PNL_PLAN_TIMING"   diagnostics on stderr,
 * and returns PNL_ERR_UNSUPPORTED for any other name: these are all the run-time switches there are.  The A/B switches of the
 * measurements in docs/CHANGELOG_kernels.md were resolved to the side that won; no build of the library reads them. */
int pnl_set_option(const char *name, const char *value);

/* Test hook (tests/test_device_math.py): the device functions of the kernel values and of the quadrature order, evaluated on
 * the current device by the production code, one thread per input.  in / out are host arrays.
 *   PNL_SELFTEST_LOG, _EXP, _EXP_RANGED   out[i] = pnl_log / pnl_exp / pnl_exp_ranged (in[i])
 *   PNL_SELFTEST_KERNEL   out[i] = kern_scale<KT>(k) kern_eval<KT, BND>(k, d2 = in[i], power tables in LDS) for the pnl_kernel
 *                         *param of dimension dim; boundary != 0: k is the folded boundary kernel of the boundary tiles and
 *                         BND = true.  path: PNL_SELFTEST_DISPATCH (+ 1: INSIDE) the KT that kern_dispatch<KT0, INSIDE> picks, KT0 = 1
 *                         for a fast kernel, else 0; any other value is the KT itself (0: exp(e ln d2) without tables, 1, 2, 3,
 *                         13, 14, 15, 17); the kernel must suit that path (fast for 1, 2 and >= 10)
 *   PNL_SELFTEST_SCALING  out[i] = pw_scaling<dim>(W, s = in[i], boundary), W from the pnl_order_function *param
 *   PNL_SELFTEST_QORDER   in[4 i ..] = h1, h2, d2, H0 of a cell pair; out[3 i ..] = quad_order_exact, quad_order_try,
 *                         quad_order_fast for the pnl_order_formula *param, ln h and |ln(h / H0)| staged like the tile kernels
 *   PNL_SELFTEST_SETTLED_LAYOUT   host only, no device: in[i] = 8 tid + k names sweep k < 8 of thread tid < 512 of the mixed-tile
 *                         kernel over a tile of 64 x 64 cell pairs; out[3 i ..] = pair index p, cell i of block a, cell j of block b.
 *                         The 2-bit code of that pair is in bits 2 k, 2 k + 1 of word tid of a settled tile's codes */
enum { PNL_SELFTEST_LOG = 0, PNL_SELFTEST_EXP = 1, PNL_SELFTEST_EXP_RANGED = 2, PNL_SELFTEST_KERNEL = 3, PNL_SELFTEST_SCALING = 4,
       PNL_SELFTEST_QORDER = 5, PNL_SELFTEST_SETTLED_LAYOUT = 6 };
#define PNL_SELFTEST_DISPATCH 100
int pnl_selftest(int op, int path, int dim, int boundary, const void *param, int n, const double *in, double *out);

/* ---- lifetime ---------------------------------------------------------------- */
int pnl_create(int device_id, pnl_context **ctx);
void pnl_destroy(pnl_context *ctx);
const char *pnl_error_string(pnl_context *ctx);
const char *pnl_version(void);
/* use a caller-owned HIP stream (hipStream_t) for all later work; NULL = the context's own stream */
int pnl_set_stream(pnl_context *ctx, void *hip_stream);
int pnl_synchronize(pnl_context *ctx);

/* ---- problem description (replaces setMesh1/2 + precomputeSimplices, NO:111-191) ---------- */
/* vertices[nv][dim], cells[nc][dim+1], vol[nc], h[nc] (mesh.volVector / hVector), H0 = diam/sqrt(8) */
int pnl_upload_mesh(pnl_context *ctx, int dim, int nv, const double *vertices_host, int nc, const int32_t *cells_host,
                    const double *vol_host, const double *h_host, double H0);
/* Cells renumbered by the host (spatial locality, label-following blocks): orig[nc] = the caller's number of every uploaded cell.
 * Touching pairs then keep the orientation the reference's loop gives them -- cellNo1 <= cellNo2 in the CALLER's numbering decides
 * which cell is the first argument of the singular rule (NA:1386-1396) -- so the operator does not depend on the renumbering
 * beyond summation order.  A cell of volume 0 without DoFs is padding inside the mesh: it forms no pair and is not counted.
 * orig = NULL: the numbering of the upload. */
int pnl_set_cell_order(pnl_context *ctx, int nc, const int32_t *orig_host);
/* Interaction set = a linear image of the l2 ball: the kernel sees |T (x - y)| instead of |x - y| (ellipse_retriangulation /
 * ellipse_barycenter = linearTransformInteraction over ball2, interactionDomains.pyx:1393-1630; T = [[cos t / a, -sin t / a],
 * [sin t / b, cos t / b]] row-major, 2D).  Quadrature points and the cut-element geometry are formed in the transformed
 * coordinates; cell volumes, h and the centre distance of the order formula stay those of the mesh.  NULL: identity. */
int pnl_set_interaction_transform(pnl_context *ctx, int dim, const double *T_host);
/* dofs[nc][dpe] (negative = boundary DoF, dm.dofs), dof_perm_table[(dim+1)!][dpe]
 * (precomputedDoFPermutations, NO:66-109) */
int pnl_upload_dofmap(pnl_context *ctx, int dpe, int dofs_per_vertex, int dofs_per_edge, int num_dofs,
                      const int32_t *dofs_host, const int32_t *dof_perm_table_host);
/* Variable fractional order that is piecewise constant per element pair (Kernel.evalParams at the two cell centres,
 * NO:509-513, kernelsCy.pyx:1852-1867; order functions fractionalOrders.pyx:203-336, 826-882): the order takes nclasses
 * distinct values.  cell_labels[nc] / facet_labels[nb] (boundary facets, may be NULL without zeroExterior) are the labels
 * of the centres, cls_of[num_labels][num_labels] the class of a label pair.  After this call pnl_select_class(k) makes
 * pnl_set_kernel / pnl_set_order_formula / pnl_upload_singular_rule act on class k (kernel parameters, order formula and
 * the near rules keyed by the class's singularity, FL2:664/688).  nclasses = 1, num_labels = 0 restores a constant order. */
int pnl_set_classes(pnl_context *ctx, int nclasses, int num_labels, const int32_t *cell_labels_host,
                    const int32_t *facet_labels_host, const int32_t *cls_of_host);
/* The order table of pnl_set_classes is not symmetric, s(label1, label2) != s(label2, label1) (a piecewise-constant,
 * non-symmetric fractional order): every element pair is assembled in both orientations, each with the parameters
 * Kernel.evalParams finds for that orientation -- the symmetricCells == False branch of getDense
 * (nonlocalAssembly_{SCALAR}.pxi:1411-1428) with the fractionalLaplacian{1,2}D_nonsym local matrices, which for parameters
 * frozen per orientation reduce to the symmetric local matrix (temp == temp2 in nonlocalOperator_{SCALAR}.pxi:899-923). */
int pnl_set_nonsymmetric(pnl_context *ctx, int on);
int pnl_select_class(pnl_context *ctx, int k);
/* which = PNL_INTERIOR (gamma) or PNL_BOUNDARY (Gauss-theorem boundary kernel, KC:1982-2027) */
int pnl_set_kernel(pnl_context *ctx, int which, const pnl_kernel *kernel);
int pnl_set_order_formula(pnl_context *ctx, int which, const pnl_order_formula *formula);
/* Distant rules for orders 0..qmax (addQuadRule NO:549-600, addQuadRule_boundary NO:988-1020):
 * off[qmax+2], bary[total][3], w[total], phi[total][dpe]; facet rule foff[qmax+2], fbary[ftotal][2], fw[ftotal] */
int pnl_upload_distant_rules(pnl_context *ctx, int qmax, const int32_t *off_host, const double *bary_host,
                             const double *w_host, const double *phi_host, const int32_t *foff_host,
                             const double *fbary_host, const double *fw_host);
/* Singular rules (getNearQuadRule FL2:644-813, FL2:1255-1314, FL1:255-330, :672-712):
 * panel = -1 vertex, -2 edge, -3 face; nodes[ncoord][M] (ncoord = 2(dim+1) interior, 2dim+1 boundary),
 * w[M], psi[rows][M], fac = multiplier of vol1*vol2 (4 / -2 in 2D, 1 in 1D) */
int pnl_upload_singular_rule(pnl_context *ctx, int which, int panel, int M, int rows, const double *nodes_host,
                             const double *w_host, const double *psi_host, double fac);
/* boundary facets bcells[nb][dim] (mesh.get_surface_mesh().cells, oriented as in their cell) */
int pnl_upload_boundary(pnl_context *ctx, int nb, const int32_t *bcells_host);

/* Finite-horizon operator without a host pair list (nonlocalBuilder.getSparse, nonlocalAssembly_{SCALAR}.pxi:1062-1260): the
 * candidate cell pairs are those of the block tiles the horizon can reach, REMOTE pairs are dropped
 * (getRelativePosition, interactionDomains.pyx:875-898; nonlocalOperator_{SCALAR}.pxi:515-517), the others are integrated
 * (pairs inside the horizon tile-wise, cut pairs through the sub-simplex loops) and added without masks into the uploaded
 * pattern.  Replaces the loops
 * NA:1150-1200 over the cells of the covering cluster pairs (clusterMethodCy.pyx:4139-4194). */
int pnl_assemble_pairs_in_horizon(pnl_context *ctx, double *data, double *diag);
/* the same for the pairs whose FIRST cell lies in [cell_begin, cell_end): the reference's split of cellNo1 over ranks
 * (nonlocalAssembly_{SCALAR}.pxi:1280-1285); the parts of a partition add up to the operator (atomic adds into data / diag) */
int pnl_assemble_pairs_in_horizon_range(pnl_context *ctx, double *data_dev, double *diag_dev, int cell_begin, int cell_end);

/* ---- the hot path --------------------------------------------------------------------------- */
/* nonlocalBuilder.getDense (NA:1262-1473): accumulates the operator into A_dev[num_dofs][ldA]
 * (caller zeroes it).  Cell pairs (c1,c2), c1<=c2, with c1 in [cell_begin, cell_end) are assembled
 * (the reference's MPI split NA:1280-1285); zero_exterior adds the Omega x Omega^c term for the
 * same cells.  flags: PNL_FLAG_* below. */
#define PNL_FLAG_NO_MIRROR 1   /* leave cross contributions in A'[I,J] only (operator = A' + A'^T), for sharded matvec */
#define PNL_FLAG_SYMMETRIC_FLUSH 2   /* write every cross contribution at (I,J) and (J,I) instead of the N^2 mirror pass:
                                      * the flush work is shared by the ranks, the mirror pass is not (multi-GPU) */
int pnl_assemble_dense(pnl_context *ctx, double *A_dev, int64_t ldA, int zero_exterior, int cell_begin, int cell_end,
                       int flags);
/* Estimated cost of every block row a of the upper block triangle (tiles (a, b), b >= a, weighted by the kernel that will take them,
 * plus the per-cell work of the row's cells), for dealing contiguous block-row ranges of equal WORK over ranks
 * (tree_node.partition clusterMethodCy.pyx:1854-1896 deals by DoF count); n = number of blocks = ceil(num_cells / pnl_tile_cells) */
int pnl_block_row_costs(pnl_context *ctx, double *cost_out, int n);
/* 1 if pnl_assemble_dense with these arguments OVERWRITES every entry of A (the operator is formed in the block-slot storage and
 * folded into A in one sweep: P2 elements in 2D, whole cell range, mirrored, room for the storage), 0 if it ADDS to A and the
 * caller has to zero the matrix first (the reference allocates a zeroed matrix, NA:1262-1290), < 0 on error */
int pnl_dense_overwrites(pnl_context *ctx, int cell_begin, int cell_end, int flags);
/* Like pnl_assemble_dense but with an explicit work list of block-tile pairs for the distant pairs
 * (multi-GPU balancing): tiles[2*i] <= tiles[2*i+1] are cell-block indices, block size pnl_tile_cells().
 * Touching pairs, the Omega x Omega^c term and nothing else are restricted to c1 in [cell_begin, cell_end). */
int pnl_tile_cells(pnl_context *ctx);
int pnl_assemble_dense_tiles(pnl_context *ctx, double *A_dev, int64_t ldA, int zero_exterior, int ntiles,
                             const int32_t *tiles_host, int cell_begin, int cell_end, int flags);
/* ---- H2 near field: nonlocalBuilder.assembleClusters (NA:1663-1964) ------------------------------------------ */
/* Sparsity pattern of the near-field matrix (getSparseNearField NA:3226-3289): CSR indptr[num_dofs+1], indices[nnz],
 * column indices strictly increasing per row.  For an SSS_LinearOperator only the strict lower triangle (I > J) is
 * listed and the diagonal lives in its own vector (SSS_LinearOperator_{SCALAR}.pxi:23-60). */
int pnl_upload_sparsity(pnl_context *ctx, int nnz, const int32_t *indptr_host, const int32_t *indices_host);
/* the same with the pattern already in device memory (built there by the host layer's getSparseNearField): device-to-device
 * copies on the context's stream; only the two ends of indptr are checked -- the caller guarantees sorted, in-range rows (use
 * pnl_upload_sparsity for a validated upload) */
int pnl_upload_sparsity_device(pnl_context *ctx, int nnz, const int32_t *indptr_dev, const int32_t *indices_dev);
/* 'interior' loop over the recorded element pairs (NA:1776-1832): pairs[np][2] with c1 <= c2, masks[np][4] = the
 * 256-bit MASK_t of requested entries of the symmetric local matrix (bit k(p,q), p <= q over the 2*dpe local DoFs,
 * buildMasksForClusters NA:260-391).  Panel + quadrature as in pnl_assemble_dense; scatter = addToMatrixElemElemSymMasked
 * (NA:503-520) with the reference's addToEntry semantics: entries absent from the pattern are dropped
 * (CSR_LinearOperator_{SCALAR}.pxi:150-170), SSS keeps I >= J only (SSS_LinearOperator_{SCALAR}.pxi:104-130).
 * data_dev[nnz] (+ diag_dev[num_dofs] for SSS, NULL for CSR) are accumulated into; the caller zeroes them. */
/* masks == NULL: every entry of every pair is requested */
int pnl_assemble_pairs_masked(pnl_context *ctx, int np, const int32_t *pairs_host, const uint64_t *masks_host,
                              double *data_dev, double *diag_dev);
/* Gauss-theorem boundary term over explicit items: the cluster-local term (NA:1842-1889; facets = boundary of
 * cellsUnion, nonlocalAssembly.pyx:505-578) and the global Omega x Omega^c term with fac = +-1 (NA:1896-1913, 1945-1964).
 * cells[ni], facets[ni][dim] vertex ids oriented as in their owning cell, masks[ni] bit field over the dpe(dpe+1)/2
 * entries (getElemSymMaskCluster NA:463-478), scatter addToMatrixElemSymMasked NA:534-546 times fac. */
int pnl_assemble_boundary_masked(pnl_context *ctx, int ni, const int32_t *cells_host, const int32_t *facets_host,
                                 const uint32_t *masks_host, double fac, double *data_dev, double *diag_dev);
/* Tiled near-field assembly: the same operator as pnl_assemble_pairs_masked + pnl_assemble_boundary_masked over all
 * cluster pairs (assembleClusters NA:1663-1964), organised for the GPU instead of element pair by element pair.  The host
 * (clusters.nearFieldPlan) lists, per UNORDERED near-field cluster pair {n1, n2} (pair_nodes; nodes = sorted DoF lists
 * node_off / node_dofs): tiles (64-cell chunk of n1.cells) x (chunk of n2.cells) -- chunk tables: cells (-1 = padding),
 * the chunk's DoFs that belong to the node and the slot of every local DoF in that list --; a slot in the diagonal-block
 * buffer for every cell of cellsInter (d_cell, d_pair; tile_dslotA/B give the slot of a tile's cells or -1); the
 * touching element pairs (sing_items[common vertices - 1] = (pair, c1 <= c2)); the facets of the boundary of cellsUnion
 * (pair_foff, fvid) and the touching (cell, facet) items of the cluster-local Gauss-theorem term (bt_slot, bt_cell,
 * bt_facet).  tile_flags bit 0: n1 == n2.  No masks cross the boundary: an entry of a local matrix is kept iff its DoF pair
 * {I, J} belongs to the cluster pair ((I in n1, J in n2) or (I in n2, J in n1)), and is written at (I, J) and (J, I) with the
 * addToEntry semantics of the uploaded pattern.  Constant order, infinite horizon.  cluster_boundary = 0 skips the
 * Gauss-theorem term. */
typedef struct {
    int32_t npairs, nnodes, nchunks, chunk_stride, ntiles, num_dslots, nfacets, tile;
    const int32_t *pair_nodes, *node_off, *node_dofs;
    const int32_t *chunk_cells, *chunk_ndof, *chunk_dofs;
    const int16_t *chunk_slot;
    const int32_t *tile_chunkA, *tile_chunkB, *tile_pair, *tile_flags, *tile_dslotA, *tile_dslotB;
    const int32_t *d_cell, *d_pair;
    int32_t n_sing[3];
    int32_t n_btouch;
    const int32_t *sing_items[3];
    const int32_t *pair_foff, *fvid;
    const int32_t *bt_slot, *bt_cell, *bt_facet;
} pnl_cluster_plan;
int pnl_assemble_clusters_tiled(pnl_context *ctx, const pnl_cluster_plan *plan, int cluster_boundary, double *data_dev,
                                double *diag_dev);
/* ---- H2 far field (clusterMethodCy.pyx) -----------------------------------------------------------------------------
 * Cluster tree (nodes with parent, level, box), its leaves (sorted DoFs, cells touching them), the admissible cluster pairs
 * far[nfar][2] = (n1, n2) (getAdmissibleClusters :4046-4136), one interpolation order m for all nodes, the transfer
 * operators transfer[node][M][M] (row: tensor index on the parent's Chebyshev grid; transferMatrixBuilder :2004-2073; unused
 * for the root) and a volume quadrature rule for the leaf values.  pnl_h2_setup evaluates on the device the kernel
 * interpolants -2 gamma(xi_i, eta_j) of every admissible pair (assembleFarFieldInteractions :2153-2238) and the leaf values
 * int phi_I L_alpha (enterLeafValues :1205-1325).  pnl_h2_matvec adds the far field to y: upward pass, interactions,
 * downward pass (H2Matrix.matvec :2269-2295 without the near-field term, which is pnl_spmv).  A kernel with a finite horizon (l2 ball)
 * is taken if every admissible pair lies inside the horizon (pnl_tree_build_horizon).  Tensor index
 * alpha = alpha_0 + m alpha_1 (coordinate 0 fastest), M = m^dim. */
typedef struct {
    int32_t nnodes, nleaves, nfar, m, nlevels, nq;
    const double *box;
    const int32_t *parent, *level;
    const int32_t *leaf_node, *leaf_dof_off, *leaf_dofs, *leaf_cell_off, *leaf_cells;
    const int32_t *far;
    const double *transfer;
    const double *qbary, *qw, *qphi;
    /* variable order (pnl_set_classes): kernel class of every admissible pair -- the order between the kernel blocks of its two
     * clusters (the reference evaluates the variable kernel at the interpolation points, clusterMethodCy.pyx:2213); NULL for a
     * constant order */
    const int32_t *far_class;
    /* 1: the leaves cover only a part of the DoFs (a rank's own subtrees; DistributedH2Matrix_localData clusterMethodCy.pyx:3368-3920):
     * the upward pass reads x, and the downward pass adds to y, at the DoFs of these leaves only; 0: the leaves partition the DoFs */
    int32_t partial_leaves;
} pnl_h2_plan;
int pnl_h2_setup(pnl_context *ctx, const pnl_h2_plan *plan);
int pnl_h2_matvec(pnl_context *ctx, const double *x_dev, double *y_dev);
/* The phases of pnl_h2_matvec on caller-owned coefficient arrays cup / cdown [nnodes][M] (device memory), for operators that exchange
 * cluster coefficients between ranks instead of vector entries (communicateFar, clusterMethodCy.pyx:3610-3647):
 *   pnl_h2_upward    cup = 0; leaves of the plan: cup[leaf] = V^T x; then level by level cup[parent] += T cup[child]
 *   pnl_h2_interact  cdown = 0; cdown[n1] += K cup[n2] over the plan's admissible pairs
 *   pnl_h2_downward  level by level cdown[child] += T^T cdown[parent]; y[dofs of the plan's leaves] += V cdown[leaf]
 * pnl_h2_sizes: out2 = (number of nodes, M) */
int pnl_h2_upward(pnl_context *ctx, const double *x_dev, double *cup_dev);
int pnl_h2_interact(pnl_context *ctx, const double *cup_dev, double *cdown_dev);
int pnl_h2_downward(pnl_context *ctx, double *cdown_dev, double *y_dev);
int pnl_h2_sizes(pnl_context *ctx, int32_t *out2);
/* what an H2 operator file stores besides the tree (H2Matrix.HDF5write / HDF5read, clusterMethodCy.pyx:2449-2550): which = 0 the
 * kernel interpolants K[nfar][M][M] of the plan's admissible pairs, which = 1 the leaf values, V_leaf[ndofs][M] of the plan's leaves
 * one after the other.  _get copies them to the host, _set replaces what pnl_h2_setup computed (an operator read from a file) */
int pnl_h2_get(pnl_context *ctx, int which, double *dst_host);
int pnl_h2_set(pnl_context *ctx, int which, const double *src_host);
/* The far field for a block of vectors, free of floating-point atomics (csrc/pnl_h2_block.hip).  Vectors are stored one per row as in
 * pnl_gemv_block: vector v is X_dev[v*ldx .. v*ldx + N), its result Y_dev[v*ldy .. v*ldy + N), N the number of DoFs.  Coefficient
 * blocks cupB / cdownB are [nnodes][M][16] doubles with the vector index fastest.  The mathematics is that of the single-vector phases:
 *   pnl_h2_upward_block    cupB is OVERWRITTEN: 0; leaves of the plan: cupB[leaf][.][v] = V^T X[v]; then level by level from the deepest
 *                          cupB[parent] += T_child cupB[child].  X is read at the DoFs of the plan's leaves only (partial_leaves).
 *   pnl_h2_interact_block  cdownB is OVERWRITTEN: cdownB[n1] = sum over the plan's pairs (n1, n2) of K_pair cupB[n2]; 0 without a pair.
 *   pnl_h2_downward_block  cdownB is MODIFIED IN PLACE: level by level from the root cdownB[child] += T_child^T cdownB[parent]; then
 *                          Y[v][dofs of the leaf] += V cdownB[leaf][.][v].  Y is ADDED to, at the DoFs of the plan's leaves only.
 *   pnl_h2_matvec_block    the three phases on the context's own cupB / cdownB (grown once): Y[v] += far field of X[v].  Any nvec >= 1,
 *                          in groups of at most 16, one pass over K, T and V per group (nvec = 17 costs two passes).
 * The slots v >= nvec of cupB and cdownB are zero after the calls.  The padding of X and Y (ld > N) is neither read into a sum nor
 * written.  The contraction runs on v_mfma_f64_16x16x4_f64, 16 rows of an M x M block being the A operand and the vectors the 16-wide
 * B operand (vectors that do not exist are zero operands).  One workgroup per DESTINATION node, NO floating-point atomics: every sum
 * has a shape fixed by the plan -- a leaf adds its DoFs in ascending order, a parent its children in ascending node number, n1 its
 * pairs in ascending pair index, and every child and every leaf DoF has one writer.  The bits of Y[v] depend on the plan, on K, V, T,
 * X[v] and the old Y[v] only: not on nvec, not on the position v, not on the other vectors, not on the call.  (They are not the bits
 * of pnl_h2_matvec, whose sums have another shape and an order left to the atomics.)  pnl_h2_set feeds these calls as it feeds
 * pnl_h2_matvec: they read the same K and V.  Asynchronous on the context's stream.
 * PNL_ERR_STATE without pnl_h2_setup.  PNL_ERR_INVALID, before any launch, for null pointers, nvec < 1, nvec > 16 in the three phase
 * calls, ldx < N, ldy < N, X_dev == Y_dev (cupB_dev == cdownB_dev in pnl_h2_interact_block). */
int pnl_h2_matvec_block(pnl_context *ctx, int nvec, const double *X_dev, int64_t ldx, double *Y_dev, int64_t ldy);
int pnl_h2_upward_block(pnl_context *ctx, int nvec, const double *X_dev, int64_t ldx, double *cupB_dev);
int pnl_h2_interact_block(pnl_context *ctx, const double *cupB_dev, double *cdownB_dev);
int pnl_h2_downward_block(pnl_context *ctx, int nvec, double *cdownB_dev, double *Y_dev, int64_t ldy);

/* y = A x for the uploaded pattern (CSR: diag_dev NULL; SSS: lower triangle + diagonal, y = (L + D + L^T) x):
 * CSR_LinearOperator.matvec / SSS_LinearOperator.matvec */
int pnl_spmv(pnl_context *ctx, const double *data_dev, const double *diag_dev, const double *x_dev, double *y_dev);

/* ---- non-symmetric kernels with a fractional order s(x) evaluated per quadrature point --------------------------------
 * Replaces fractionalLaplacian{1,2}D_nonsym (fractionalLaplacian2D.pyx:894-1184, fractionalLaplacian1D.pyx:410-604) with
 * piecewise == False kernels gamma(x, y) = C(s(x)) |x-y|^(-d-2 s(x)) (kernels.py:147-149, kernelsCy.pyx:596-622), the
 * non-symmetric branch of getDense (nonlocalAssembly_{SCALAR}.pxi:1411-1428, scatter :222-253) and the boundary term with
 * the pointwise boundary kernel.  P1 elements, infinite horizon.
 * type: 1 constant (p[0]), 2 smoothStep in x0, 3 linearStep in x0, 4 smoothStepRadial (fractionalOrders.pyx:338-540);
 * p = sl, sr, r, interface (radius for type 4), slope; type 5: pnl_set_order_vertex_values.  normalized: variableFractionalLaplacianScaling
 * (kernelNormalization.pyx:329-364) or 1/2. */
typedef struct pnl_order_function {
    int32_t type, normalized;
    double p[6];
    /* optional: the scaling C(s) as a Chebyshev series sum_k scal_cheb[k] T_k((s - scal_mid)/scal_half) over the range of
     * the order (a polynomial instead of two Gamma functions per quadrature point); scal_n == 0: evaluate the formula */
    int32_t scal_n, pad;
    double scal_mid, scal_half;
    double scal_cheb[32];
} pnl_order_function;

/* cell_smax[nc] / facet_smax[nb]: largest order over the centre and the vertices of a cell / boundary facet (the per-pair
 * order of Kernel.evalParamsOnSimplices, kernelsCy.pyx:1825-1846, is the max of the two); c0 / bc0: constant term of the
 * interior / boundary order formula; sing_fac / bsing_fac as in pnl_upload_singular_rule */
int pnl_set_order_function(pnl_context *ctx, const pnl_order_function *f, const double *cell_smax, const double *facet_smax,
                           double c0, double bc0, double sing_fac, double bsing_fac);
/* type 5 (feFractionalOrder / lookupExtended, fractionalOrders.pyx:541-587, 660-668): the order is a continuous P1 function on the
 * mesh of the assembly, values[nv] at its vertices.  A quadrature point is known by its cell and barycentric coordinates, so
 * s(x) = sum_k lambda_k(x) values[vertex k of the cell] needs no point location. */
int pnl_set_order_vertex_values(pnl_context *ctx, int nv, const double *values_host);
/* near rules for the nkeys distinct orders of the touching pairs (the reference keys its rule dictionary by the singularity
 * value, fractionalLaplacian2D.pyx:957): nodes[nkeys][2(dim+1) | (dim+1)+dim][M], w[nkeys][M], phi0 / phi1[nkeys][rows][M]
 * = the x and y parts of the merged-DoF shape functions (PHI3 of the reference; boundary: phi0 = PHI, phi1 unused) */
int pnl_upload_pointwise_rules(pnl_context *ctx, int which, int panel, int nkeys, int M, int rows, const double *nodes,
                               const double *w, const double *phi0, const double *phi1);
/* dense assembly; pairs[npairs][4] = (c1 <= c2 sharing `common` vertices, common, key into the near rules), bpairs[nbpairs][4]
 * = (cell, boundary facet, common, key).  Distant pairs are found and classified on the device. */
int pnl_assemble_dense_pointwise(pnl_context *ctx, double *A, int64_t ldA, int zero_exterior, int cell_begin, int cell_end,
                                 int npairs, const int32_t *pairs, int nbpairs, const int32_t *bpairs);
/* near field of these kernels: the masked element-pair loop of assembleClusters with symmetricCells == symmetricLocalMatrix == False
 * (nonlocalAssembly_{SCALAR}.pxi:1776-1840: masks over cellsUnion x cellsUnion :322-349, getElemElemMask :425-440, scatter
 * addToMatrixElemElemMasked :520-532).  pairs[np][2]: ORDERED cell pairs, each evaluated in its own orientation (swapCells is the
 * listing of (c2, c1)); masks[np][4]: bit p (2 dpe) + q of the 256-bit MASK_t requests local entry (p, q); rule[np]: -1 for a pair
 * without a common vertex (classified on the device), otherwise the key of the pair's near rule (pnl_upload_pointwise_rules);
 * data: unsymmetric CSR over the uploaded pattern (pnl_upload_sparsity), entries absent from it are dropped (addToEntry). */
int pnl_assemble_pairs_masked_pointwise(pnl_context *ctx, int np, const int32_t *pairs, const uint64_t *masks, const int32_t *rule,
                                        double *data);
/* cluster exterior of these kernels (local_matrix_surface with the pointwise boundary kernel, nonlocalAssembly_{SCALAR}.pxi:1966-2028;
 * the global Omega x Omega^c term :2126-2156 with fac = -1): items (cell, facet vertex ids[dim], mask over the dpe (dpe+1)/2 entries)
 * as pnl_assemble_boundary_masked, plus rule[ni] (-1: no common vertex, else the key of the boundary near rule) and sv[ni], the
 * largest order over the centres and vertices of cell and facet (evalParamsOnSimplices, kernelsCy.pyx:1825-1846). */
int pnl_assemble_boundary_masked_pointwise(pnl_context *ctx, int ni, const int32_t *cells, const int32_t *facets, const uint32_t *masks,
                                           const int32_t *rule, const double *sv, double fac, double *data, double *diag);

/* counters of the last assemble call (synchronises the stream) */
int pnl_get_counters(pnl_context *ctx, int64_t *out, int n);
/* device time of the last assemble call per phase in milliseconds (HIP events on the context's stream):
 * [0] general tile kernel (distant pairs, one per lane), [1] work-list kernels (high orders),
 * [2] singular pairs, [3] boundary term, [4] mirror + diagonal scatter, [5] total, [6] uniform-tile kernel. */
int pnl_get_phase_ms(pnl_context *ctx, float *out, int n);
/* The settled tiles of the resident dense tile plan (tests): tiles[i][2] = (block a, block b) of the first ntiles of them, in the order
 * of the launch (most pairs of a 6-point rule first).  Returns their number (0: the plan settles nothing), or an error. */
int pnl_get_settled_tiles(pnl_context *ctx, int32_t *tiles, int64_t ntiles);
/* Pair codes and pair lists of the first ntiles settled tiles of the resident plan (tests), in the order of pnl_get_settled_tiles; either
 * pointer may be NULL.  codes[t][512]: word tid holds the 2-bit codes of the eight pairs of thread tid (PNL_SELFTEST_SETTLED_LAYOUT).
 * lists[t][4104]: words 0 .. 2 = n4, n3, n2, the numbers of pairs of order 4, 3, 2; from word 8 on the n4 + n3 + n2 entries
 * p | (order - 2) << 12, order 4 first, then 3, then 2, ascending pair index p within an order; zero behind the last entry.
 * Returns the number of tiles the plan holds lists for (0: it keeps codes only), or an error. */
int pnl_get_settled_lists(pnl_context *ctx, uint16_t *codes, uint16_t *lists, int64_t ntiles);
/* Lane layout of the 64-cell blocks for the P1 uniform-tile kernels (2D; needs no device).  cells [nc][3] vertex ids, dofs [nc][3]
 * global DoFs (negative: none).  mode: the option PNL_UNI_LANES -- 0 identity (lane = cell, column = slot; the row stride of the
 * sub-block is the launcher's, 1 mod 32 doubles), 1 searched (default), 2 random (a bad layout; results must not depend on it).
 * sizes[4] = number of blocks, nU (largest number of DoFs of a block), row stride of the LDS sub-block in doubles (0 for mode 0),
 * padded number of cells ncp.  With the arrays NULL only sizes is filled.  lane_cell [nblocks][64]: the cell of the block lane l
 * holds; lds_col [nblocks][nU]: LDS column of a block slot; vorder [nc][3]: local vertex order of the tile kernels; cell_col [3][ncp]:
 * LDS column of (local position, cell), a trash column >= stride - 16 where the cell has no DoF; mult [nblocks]: modelled cost of a
 * sub-block add relative to a conflict-free one (mean over the 12 classes (16-lane group, local position) of the most loaded
 * double-bank; 0 for mode 0, where the bank depends on the partner block); *seconds: wall time of the layout of all blocks.
 * nthreads <= 0: the library's host-thread pool.  The tables do not depend on the number of threads. */
int pnl_uniform_lane_layout(int nc, const int32_t *cells, const int32_t *dofs, int mode, int nthreads, int32_t *sizes, uint8_t *lane_cell,
                            int16_t *lds_col, int8_t *vorder, int16_t *cell_col, double *mult, double *seconds);
/* device time of the tile kernels of the last assemble call, one HIP-event pair around each launch (milliseconds, 0 if the
 * kernel did not run; a slot that was launched several times -- order classes -- holds the sum over
 * its launches): [0] general tile kernel, [1] uniform tiles of
 * order 2, [2] order 3, [3] order 4, [4] fold + mirror of the block-slot storage, [5] work-list kernels, [6] the launch of the general
 * tile kernel over the settled tiles (part of [0]) */
enum pnl_kernel_slot { PNL_K_TILE_GENERAL = 0, PNL_K_TILE_UNIFORM2, PNL_K_TILE_UNIFORM3, PNL_K_TILE_UNIFORM4, PNL_K_FOLD_MIRROR,
                       PNL_K_WORKLIST, PNL_K_TILE_SETTLED, PNL_NUM_KERNEL_SLOTS };
int pnl_get_kernel_ms(pnl_context *ctx, float *out, int n);

/* ---- host-side planning of the H2 / near-field assembly (no GPU needed): cluster tree + admissibility
 *      (tree_node.refine clusterMethodCy.pyx:354-663 -- median splits here --, getAdmissibleClusters :4046-4136), cells of
 *      the cluster nodes (NA:2887-2898), the tile work lists of pnl_assemble_clusters_tiled (what clusters.nearFieldPlan
 *      built in numpy: chunks, tiles, touching pairs, boundary facets of cellsUnion nonlocalAssembly.pyx:540-578) and the
 *      transfer matrices of the far field (transferMatrixBuilder :2004-2073) ------------------------------------------ */
typedef struct pnl_tree pnl_tree;
typedef struct pnl_nfplan pnl_nfplan;
/* boxes[N][dim][2] support boxes of the DoFs, (d2c_ptr, d2c_idx) DoF -> cells CSR; do_admissibility: 1 tree + recursion from
 * (root, root), 0 tree only, -1 root only */
int pnl_tree_build(int N, int dim, const double *boxes, const int64_t *d2c_ptr, const int32_t *d2c_idx, int nc, double eta,
                   int min_size, int max_levels, int do_admissibility, pnl_tree **out);
/* variable order: dof_block[N] >= 0 names the kernel block of every DoF (getKernelBlocksAndJumps NA:2312-2352, the reference
 * hangs one child per block below the leaves of the partition tree, NA:2619-2640), mixed_block the block of the interface DoFs:
 * nodes with DoFs of several blocks are split by block first, only pairs of single-block nodes other than mixed_block can be
 * admissible (mixed_node, clusterMethodCy.pyx:4038) */
int pnl_tree_build_blocks(int N, int dim, const double *boxes, const int64_t *d2c_ptr, const int32_t *d2c_idx, int nc, double eta,
                          int min_size, int max_levels, int do_admissibility, const int32_t *dof_block, int mixed_block,
                          pnl_tree **out);
/* ... with the refinement type of the reference (refinementType, NA:3033-3040; tree_node.refine CM:354-663): 0 MEDIAN (the default
 * of both), 1 GEOMETRIC (the node's box is halved along its longest edge), 2 BARYCENTER (split at the mean of the DoF coordinates) */
int pnl_tree_build_refined(int N, int dim, const double *boxes, const int64_t *d2c_ptr, const int32_t *d2c_idx, int nc, double eta,
                           int min_size, int max_levels, int do_admissibility, const int32_t *dof_block, int mixed_block, int ref_type,
                           pnl_tree **out);
/* ... for a kernel with a finite horizon (getAdmissibleClusters, clusterMethodCy.pyx:4069-4090, 4115, 4131-4135, with distBoxes /
 * maxDistBoxes of the l2 ball, interactionDomains.pyx:304-337): cluster pairs farther apart than the horizon are dropped, pairs the
 * horizon may cut stay in the near field, near-field children are merged into one block only if the block fits into the horizon.
 * horizon = INFINITY: pnl_tree_build_refined */
int pnl_tree_build_horizon(int N, int dim, const double *boxes, const int64_t *d2c_ptr, const int32_t *d2c_idx, int nc, double eta,
                           int min_size, int max_levels, int do_admissibility, const int32_t *dof_block, int mixed_block, int ref_type,
                           double horizon, pnl_tree **out);
/* the same structure with refinement (MEDIAN / GEOMETRIC) and admissibility run ON THE DEVICE as level-synchronous sweeps
 * (clusterMethodCy.pyx:354-663, 4046-4136; csrc/pnl_plan_dev.hip): same nodes, same lists in the same order as pnl_tree_build_refined;
 * kernel blocks and the BARYCENTER split: PNL_ERR_UNSUPPORTED (use the host planner).  Uses the current HIP device. */
int pnl_tree_build_device(int N, int dim, const double *boxes, const int64_t *d2c_ptr, const int32_t *d2c_idx, int nc, double eta,
                          int min_size, int max_levels, int do_admissibility, int ref_type, pnl_tree **out);
void pnl_tree_destroy(pnl_tree *T);
int pnl_tree_sizes(const pnl_tree *T, int64_t *out3);                /* nodes, near pairs, far pairs */
int pnl_tree_get(const pnl_tree *T, int32_t *range, int32_t *parent, int32_t *children, int32_t *level, double *box, int32_t *perm,
                 int32_t *near, int32_t *far);
int pnl_tree_node_cells(const pnl_tree *T, int n, const int32_t *node_ids, int64_t *off, int32_t *cells);
int pnl_h2_transfer_matrices(int nnodes, int dim, int m, const double *box, const int32_t *parent, double *out);
int pnl_nfplan_build(int dim, int nv, const double *vertices, int nc, const int32_t *cells, int dpe, int N, const int32_t *dofs,
                     int nnodes, const int64_t *node_off, const int32_t *node_dofs, const int64_t *node_cell_off,
                     const int32_t *node_cells, int npairs, const int32_t *pair_nodes, int tile, int max_chunk_dofs,
                     pnl_nfplan **out);
void pnl_nfplan_destroy(pnl_nfplan *P);
int pnl_nfplan_sizes(const pnl_nfplan *P, int64_t *out9);
int pnl_nfplan_get(const pnl_nfplan *P, int which, void *dst);

/* sparsity pattern of a finite-horizon operator (getSparse NA:1062-1260): the DoF pairs (I, J) for which a cell holding I and
 * a cell holding J have a vertex pair closer than delta (the pairs getRelativePosition does not call REMOTE,
 * interactionDomains.pyx:875-898); strict_lower: only J < I (SSS storage).  Rows sorted, CSR through the getters. */
typedef struct pnl_pattern pnl_pattern;
int pnl_horizon_pattern(int dim, int nv, const double *vertices, int nc, const int32_t *cells, int dpe, int N, const int32_t *dofs,
                        double delta, int strict_lower, pnl_pattern **out);
/* pattern of the near field of the cluster pairs pairs[npairs][2] (node ids of the tree): union of the blocks n1.dofs x n2.dofs,
 * getSparseNearField NA:3226-3289; strict_lower keeps I > J (SSS) */
int pnl_near_pattern(const pnl_tree *T, int npairs, const int32_t *pairs, int strict_lower, pnl_pattern **out);
/* The row pointer of a pattern is int32 (the reference's INDEX_t; pnl_upload_sparsity and the CSR / SSS operators index with
 * it): both builders return PNL_ERR_UNSUPPORTED for a pattern with more stored entries than the limit instead of wrapping.
 * pnl_pattern_set_max_nnz lowers the limit (process-wide, 1 ... 2^31 - 1; other values leave it unchanged) and returns the old one. */
int64_t pnl_pattern_set_max_nnz(int64_t max_nnz);
int64_t pnl_pattern_nnz(const pnl_pattern *P);
int pnl_pattern_get(const pnl_pattern *P, int32_t *indptr, int32_t *indices);
void pnl_pattern_destroy(pnl_pattern *P);

/* ---- row slab of a rank: distributed dense operator (the reference's DistributedH2Matrix_globalData.matvec,
 *      clusterMethodCy.pyx:3127-3154, on a row partition, tree_node.partition :1854-1896) ------------------------------
 * After pnl_set_row_slab the dense assemble calls write ONE-SIDED into a slab of nrows x ncols doubles (leading dimension
 * ldA >= ncols): row r holds global DoF rowdofs[r], column j global DoF coldofs[j] (both increasing); cross blocks at (c1's
 * DoF, c2's DoF) for c1 < c2, the symmetric local matrices of touching pairs once at (min, max); no mirror pass; the
 * per-cell diagonal blocks stay in the per-cell buffer (pnl_get_diag_blocks: 2 x ncp x ND doubles, the rank's partial
 * sums over ALL cells).  The rows must contain every DoF of the cells in the caller's cell range and of the cells touching
 * them, the columns every DoF of the cells from cell_begin on.  The rank's part of the operator is
 * A' + A'^T - diag(A') + scatter(D); pnl_slab_matvec applies it (y is overwritten; the caller all-reduces y over the
 * ranks).  nrows = 0 restores the full N x N output. */
int pnl_set_row_slab(pnl_context *ctx, int nrows, const int32_t *rowdofs_host, int ncols, const int32_t *coldofs_host);
int pnl_diag_blocks_size(pnl_context *ctx);
int pnl_get_diag_blocks(pnl_context *ctx, double *dst_dev);
int pnl_slab_matvec(pnl_context *ctx, const double *slab_dev, int64_t ld, const double *diag_blocks_dev, const double *x_dev,
                    double *y_dev);
int pnl_slab_diagonal(pnl_context *ctx, const double *slab_dev, int64_t ld, const double *diag_blocks_dev, double *diag_dev);

/* ---- adjacent solve path: Dense_LinearOperator.matvec (dgemv, DenseLinearOperator_{SCALAR}.pxi:14-18)
 *      and cg_solver + jacobi (base/PyNucleus_base/solvers.pyx:363-444, 229-245) ------------------- */
/* y = A x (n x n, row-major, leading dimension ldA); symmetric_half = 1: y = (A + A^T) x for PNL_FLAG_NO_MIRROR storage;
 * symmetric_half = 2: A is stored in full and is symmetric -- the upper triangle is read once for both A x and A^T x (4 n^2 bytes
 * instead of 8 n^2: a GEMV is bound by HBM).  pnl_cg_jacobi always reads the upper triangle (CG needs a symmetric operator). */
int pnl_gemv(pnl_context *ctx, const double *A_dev, int64_t ldA, int n, const double *x_dev, double *y_dev,
             int symmetric_half);
/* Jacobi-preconditioned CG on A x = b; x_dev holds the initial guess and the result.
 * Stops when ||r||_2 <= tol (absolute, like the reference's default) or after maxiter; returns iterations in
 * *iters and the final residual norm in *residual. */
int pnl_cg_jacobi(pnl_context *ctx, const double *A_dev, int64_t ldA, int n, const double *b_dev, double *x_dev,
                  double tol, int maxiter, int *iters, double *residual);

/* ---- solver side on the device: geometric multigrid over a hierarchy of assembled nonlocal operators
 *      (fractionalLevel, nl/PyNucleus_nl/helpers.py:312-380), multigrid-preconditioned CG, theta time stepping -----------
 * y = alpha A x + beta b for a dense row-major nrows x ncols block (LinearOperator.residual = (alpha, beta) = (-1, 1);
 * b_dev may be y_dev) and y = alpha A x + beta y for a CSR matrix on the device (restriction / prolongation
 * multilevelSolver/PyNucleus_multilevelSolver/restriction_*_P1.pxi, mass matrix). */
int pnl_gemv_axpby(pnl_context *ctx, const double *A_dev, int64_t ldA, int nrows, int ncols, const double *x_dev, double alpha,
                   double beta, const double *b_dev, double *y_dev);
int pnl_csr_matvec(pnl_context *ctx, int nrows, const int32_t *indptr_dev, const int32_t *indices_dev, const double *data_dev,
                   const double *x_dev, double alpha, double beta, double *y_dev);
/* One level of the hierarchy, level 0 = coarsest (multigrid_{SCALAR}.pxi:86-135 levelMemory: A, R, P): the dense operator and
 * its diagonal (Jacobi smoother, smoothers_{SCALAR}.pxi:118-131), the restriction to the next coarser level (n_coarse x n)
 * and the prolongation from it (n x n_coarse) as CSR arrays on the device (unused on level 0, where only n counts). */
typedef struct {
    int32_t n;
    int32_t pad;
    const double *A_dev;
    int64_t ldA;
    const double *diag_dev;
    const int32_t *R_indptr_dev, *R_indices_dev;
    const double *R_data_dev;
    const int32_t *P_indptr_dev, *P_indices_dev;
    const double *P_data_dev;
    /* kind 0: the dense operator A_dev.  kind 1 (the FINEST level only): the H2 operator currently set up in the context
     * (pnl_h2_setup): near field as full CSR (near_*_dev, n rows) + the far field through pnl_h2_matvec; A_dev is unused,
     * diag_dev = the diagonal of the near field.  The hierarchies of the reference's drivers put H2 operators on the fine
     * levels (helpers.py:312-380 with matrixFormat 'H2').  kind 2: the dense operator A_dev is SYMMETRIC and stored in full; its
     * products read the upper triangle only (the two-sided sweep of pnl_gemv with symmetric_half = 2). */
    int32_t kind, pad2;
    const int32_t *near_indptr_dev, *near_indices_dev;
    const double *near_data_dev;
} pnl_mg_level_desc;
typedef struct pnl_mg pnl_mg;
/* multigrid.__init__ / setup (:86-235): V cycle, Jacobi smoother with damping omega and presmooth / postsmooth sweeps
 * (defaults of the reference: 2/3, 1, 1), coarse solver = multiplication with the inverse of the coarsest operator
 * (coarse_inverse_dev, n_0 x n_0 row-major; the reference factorises it with LU).  The level arrays stay owned by the caller
 * and must outlive the object. */
int pnl_mg_create(pnl_context *ctx, int nlevels, const pnl_mg_level_desc *levels, const double *coarse_inverse_dev, double omega,
                  int presmooth, int postsmooth, pnl_mg **out);
int pnl_mg_destroy(pnl_mg *mg);
/* one cycle on the finest level (solveOnLevel :237-292); x_is_zero: the first residual is b (simpleResidual) */
int pnl_mg_cycle(pnl_mg *mg, const double *b_dev, double *x_dev, int x_is_zero);
/* multigrid.solve (:296-390): cycles until ||b - A x||_2 <= tol or maxiter; residuals[0..min(iters+1, cap)) = the norms */
int pnl_mg_solve(pnl_mg *mg, const double *b_dev, double *x_dev, double tol, int maxiter, int x_is_zero, int *iters, double *residuals,
                 int residuals_cap);
/* cg_solver.solve (base/PyNucleus_base/solvers.pyx:363-444) preconditioned by one cycle (multigridPreconditioner :470-497);
 * A_dev NULL: the finest operator of the hierarchy; convergence on sqrt(r.Br) like the reference */
int pnl_mg_cg(pnl_mg *mg, const double *A_dev, int64_t ldA, const double *b_dev, double *x_dev, double tol, int maxiter, int x_is_zero,
              int *iters, double *residuals, int residuals_cap);
/* CrankNicolson.step (base/PyNucleus_base/timestepping.py:93-112) for M u_t + S u = g:
 * (M/dt + theta S) u_new = (M/dt) u - (1-theta) S u + forcing, forcing = (1-theta) g(t) + theta g(t+dt) (setRHS :76-91),
 * solved by pnl_mg_cg on the hierarchy mg of M/dt + theta S from the initial guess u (u_dev is overwritten). */
int pnl_theta_step(pnl_mg *mg, const double *S_dev, int64_t ldS, const int32_t *M_indptr_dev, const int32_t *M_indices_dev,
                   const double *M_data_dev, double dt, double theta, const double *forcing_dev, double *u_dev, double tol, int maxiter,
                   int *iters, double *residual);
/* 1/diag(A) into dinv_dev (jacobi_solver.setup, solvers.pyx:233-237) */
int pnl_inv_diagonal(pnl_context *ctx, const double *A_dev, int64_t ldA, int n, double *dinv_dev);
/* Jacobi-preconditioned CG on (scale M) x = b for a CSR matrix on the device (n rows, symmetric positive definite, the diagonal
 * stored): the loop of pnl_cg_jacobi -- same update order, convergence on sqrt(r.Br) <= tol, residual recomputed every 50
 * iterations -- with the product of pnl_csr_matvec.  What the reference does with `cg-jacobi` on the mass matrix
 * (solverBuilder(t, 1., 0.), timestepping.py:377-682).  x_dev holds the initial guess unless x_is_zero, and the result. */
int pnl_csr_cg_jacobi(pnl_context *ctx, int n, const int32_t *indptr_dev, const int32_t *indices_dev, const double *data_dev, double scale,
                      const double *b_dev, double *x_dev, double tol, int maxiter, int x_is_zero, int *iters, double *residual);

/* ---- pointwise nonlinearities against the test functions (csrc/pnl_reaction.hip): assembleNonlinearity
 *      (fem/PyNucleus_fem/femCy.pyx:3087-3178) on the device ----------------------------------------------------------------------
 * A space is the cell -> DoF table dofs[ncells][dofs_per_cell] (negative: no DoF, its value counts as 0), the cell volumes
 * vol[ncells] and a volume rule: phi[dofs_per_cell][nq] = the local shape functions at the nq <= 7 nodes, w[nq] (summing to 1).
 * dofs_per_cell = 2, 3 or 6.  The space owns the inverted index DoF -> (cell, local index) in ascending cell order and the
 * workspace of the local contributions. */
typedef struct pnl_fe_space pnl_fe_space;
int pnl_fe_space_create(pnl_context *ctx, int ncells, int dofs_per_cell, int nq, int ndofs, const int32_t *dofs_host, const double *vol_host,
                        const double *phi_host, const double *w_host, pnl_fe_space **out);
int pnl_fe_space_destroy(pnl_fe_space *space);
/* PNL_FUN_BRUSSELATOR (2 -> 2, params B, Q): z = B u + Q^2 v + (B/Q) u^2 + 2 Q u v + u^2 v, f = (-u + z, -z) (femCy.pyx:3025-3041);
 * PNL_FUN_CUBIC (1 -> 1, no params): u^3 - u (CahnHilliard_F_prime) */
enum pnl_function { PNL_FUN_BRUSSELATOR = 0, PNL_FUN_CUBIC = 1 };
/* R = beta R + alpha N(U),  N(U)[o][I] = sum over (c, m) with dof(c, m) = I of vol_c sum_q w_q f_o(u(c, q)) phi_m(xi_q),
 * u_j(c, q) = sum_m U[j][dof(c, m)] phi_m(xi_q).  U_dev[nin][ldU], R_dev[nout][ldR], ldU, ldR >= ndofs.  No float atomics: the
 * same input gives the same bits.  PNL_ERR_INVALID for an unknown function or nin / nout / nparams that are not the function's.
 * Asynchronous on the context's stream. */
int pnl_assemble_nonlinearity(pnl_fe_space *space, int fun, const double *params_host, int nparams, int nin, const double *U_dev,
                              int64_t ldU, int nout, double alpha, double beta, double *R_dev, int64_t ldR);

/* ---- IMEX Runge-Kutta for  m_c M u_c' + S u_c - N_c(u) = g_c(t),  c < ncomp  (IMEX._stepOfPicard, timestepping.py:377-682;
 *      signs as there: E = -N(U), I = S U) ---------------------------------------------------------------------------------------
 * Tableau AE, AI [s][s] row-major (AE strictly lower, AI lower triangular, one value gamma on the diagonal of AI at the stages
 * that are solved), bE, bI [s].  S_dev: the dense symmetric operator, M: the CSR mass matrix, both shared by the components;
 * fun / params: the nonlinearity, its number of inputs = outputs = ncomp.  solver PNL_IMEX_CG_MG: mg[c] is the multigrid object
 * on the hierarchy of m_c M + dt gamma S (pnl_mg_cg to tol / maxiter); PNL_IMEX_CHOL: chol_dev[c] / ldchol[c] is the Cholesky
 * factor of that matrix (pnl_potrf; pnl_potrs).  mass_tol / mass_maxiter: the mass solve at the end of a sweep
 * (pnl_csr_cg_jacobi).  All device arrays stay owned by the caller and must outlive the object. */
#define PNL_IMEX_MAX_STAGES 4
#define PNL_IMEX_MAX_COMP 2
enum { PNL_IMEX_CG_MG = 0, PNL_IMEX_CHOL = 1 };
typedef struct {
    int32_t s, ncomp, n, fun, nparams, solver, maxiter, mass_maxiter;
    double AE[PNL_IMEX_MAX_STAGES*PNL_IMEX_MAX_STAGES], AI[PNL_IMEX_MAX_STAGES*PNL_IMEX_MAX_STAGES];
    double bE[PNL_IMEX_MAX_STAGES], bI[PNL_IMEX_MAX_STAGES];
    double mass_scale[PNL_IMEX_MAX_COMP], params[4];
    double dt, tol, mass_tol;
    const double *S_dev;
    int64_t ldS;
    const int32_t *M_indptr_dev, *M_indices_dev;
    const double *M_data_dev;
    pnl_fe_space *space;
    pnl_mg *mg[PNL_IMEX_MAX_COMP];
    const double *chol_dev[PNL_IMEX_MAX_COMP];
    int64_t ldchol[PNL_IMEX_MAX_COMP];
} pnl_imex_desc;
typedef struct pnl_imex pnl_imex;
int pnl_imex_create(pnl_context *ctx, const pnl_imex_desc *desc, pnl_imex **out);
int pnl_imex_destroy(pnl_imex *imex);
/* One sweep (u_prev, u) -> u_new with the vectors [ncomp][n] in HBM.  Stage k: U_k = u if row k of AE is zero, else per component
 *   (m_c M + dt gamma S) U_k = m_c M u_prev - dt sum_{j<k} (AE[k][j] E_j + AI[k][j] I_j) + dt sum_{j<=k} AI[k][j] g_j
 * from the initial guess u; E_k = -N(U_k) and I_k = S U_k are formed only if a later stage or the final update uses them.  Then
 *   m_c M u_new = m_c M u_prev - dt sum_k (bE[k] E_k + bI[k] I_k) + dt sum_k bI[k] g_k
 * from the initial guess u.  u_dev receives u_new; u_prev_dev may be u_dev (a plain step).  force_dev: g as [s][ncomp][n], or NULL.
 * iters_out (host, may be NULL): [(s + 1) ncomp] iterations of the stage solves [k][c], then of the mass solves [c].  The
 * right-hand sides are formed by one kernel each from the stored rows; stage storage is one block owned by the object. */
int pnl_imex_sweep(pnl_imex *imex, const double *u_prev_dev, double *u_dev, const double *force_dev, int32_t *iters_out);

/* ---- direct solver for the dense symmetric positive definite operators (csrc/pnl_direct.hip): what lu_solver.setup / solve
 *      (base/PyNucleus_base/solvers.pyx:80-186: dense copy, getrf, getrs) is for `--matrixFormat dense --solver lu`.  The operators
 *      of the symmetric kernels are positive definite, so the factor is Cholesky; pnl_getrf / pnl_getrs below are the LU. -------
 * replaces lu_solver.setup (solvers.pyx:80-186): A = L L^T in place on the lower triangle of the row-major n x n block A_dev
 * (leading dimension ldA >= n).  Reads A[i][j] for j <= i only and leaves L there, L[i][i] > 0; nothing above the diagonal and
 * nothing in the padding columns n .. ldA - 1 is read or written.  *info = 0 on success; *info = k > 0 if the leading minor of
 * order k is not positive definite (pivot k is not > 0, NaN included): the call still returns PNL_OK, the lower triangle is then
 * unspecified and everything else untouched.  PNL_ERR_INVALID for n < 0, ldA < n or a null pointer with n > 0; n = 0 is a no-op.
 * Runs on the context's stream and synchronises it to return info (the pivot check costs no synchronisation per panel). */
int pnl_potrf(pnl_context *ctx, double *A_dev, int64_t ldA, int n, int *info);
/* replaces lu_solver.solve (solvers.pyx:80-186): L y = b, then L^T x = y, in place on the nrhs >= 1 right-hand sides
 * B_dev[r * ldb .. r * ldb + n), ldb >= n, with the factor pnl_potrf left in the lower triangle of L_dev (only that triangle is
 * read).  Asynchronous on the context's stream. */
int pnl_potrs(pnl_context *ctx, const double *L_dev, int64_t ldL, int n, double *B_dev, int64_t ldb, int nrhs);

/* ---- direct solver for the dense operators that are not symmetric (csrc/pnl_direct.hip): lu_solver.setup / solve as they stand, getrf
 *      and getrs, for the orders evaluated per quadrature point. ------------------------------------------------------------------
 * replaces lu_solver.setup: P A = L U with partial pivoting in place on the row-major n x n block A_dev (leading dimension
 * ldA >= n).  The strict lower triangle receives L (unit diagonal, not stored, every |l_ik| <= 1), the upper triangle with the
 * diagonal U.  piv_dev[k], k < n, is 0-based with k <= piv_dev[k] < n: LAPACK's swap sequence (at step k the rows k and piv_dev[k] of
 * the whole matrix were exchanged).  The pivot of column k is the entry of largest magnitude among the rows k .. n - 1 as they stand
 * at that step, the lowest row among equal magnitudes; the search is a deterministic reduction, so the same input gives the same
 * bits and the same piv_dev.  *info = 0, or the 1-based index of the first column whose pivot p does not satisfy |p| > 0 (NaN
 * included): the call still returns PNL_OK and the block is then unspecified.  The padding columns n .. ldA - 1 are neither read
 * nor written.  PNL_ERR_INVALID for n < 0, ldA < n or a null pointer with n > 0; n = 0 is a no-op.  Runs on the context's stream
 * and synchronises it to return info. */
int pnl_getrf(pnl_context *ctx, double *A_dev, int64_t ldA, int n, int32_t *piv_dev, int *info);
/* replaces lu_solver.solve: the swaps applied to b, L y = P b (unit diagonal, no division), U x = y, in place on the nrhs >= 1
 * right-hand sides B_dev[r * ldb .. r * ldb + n), ldb >= n, with the factors and the swap sequence pnl_getrf left.  A block of
 * right-hand sides gives the bits of the one-by-one solves.  Asynchronous on the context's stream. */
int pnl_getrs(pnl_context *ctx, const double *LU_dev, int64_t ldLU, int n, const int32_t *piv_dev, double *B_dev, int64_t ldb, int nrhs);

/* ---- linear combinations of dense blocks (csrc/pnl_interp.hip): the operators interpolated in the fractional order,
 *      interpolationOperator (base/PyNucleus_base/linear_operators.pyx:1261-1391): A(s) = sum_k w_k(s) A(s_k) over the operators at the
 *      Chebyshev nodes of an interval. ---------------------------------------------------------------------------------------------
 * A_dev: HOST array of m device pointers to row-major nrows x ncols blocks with the common leading dimension ldA >= ncols;
 * coeffs_host[m].  Pointers and coefficients travel in the kernel arguments: no upload, no allocation, no synchronisation per call;
 * both calls are asynchronous on the context's stream.  The combined entry is t = c_0 a_0, then t = fma(c_k, a_k, t) in ascending k; the
 * product then accumulates fma(t, x[c], acc).  All reductions have a fixed shape and use no floating-point atomics: the same input
 * gives the same bits, whatever the alignment (16-byte loads and stores where the pointers and leading dimensions allow them, scalar
 * ones otherwise).  PNL_ERR_INVALID, before any launch, for m < 1, m > PNL_INTERP_MAX_OPS, a null pointer (an entry of A_dev included),
 * nrows or ncols < 1, a leading dimension below ncols, B_dev equal to an A_dev[k], x_dev equal to y_dev. */
#define PNL_INTERP_MAX_OPS 21     /* M_max + 1 of the node selection */
/* B[r][c] = sum_k coeffs[k] A_k[r][c] for r < nrows, c < ncols; the columns ncols .. ldB - 1 of B are not written */
int pnl_lincomb(pnl_context *ctx, int m, const double *const *A_dev, int64_t ldA, int nrows, int ncols, const double *coeffs_host,
                double *B_dev, int64_t ldB);
/* y = alpha (sum_k coeffs[k] A_k) x + beta b with the conventions of pnl_gemv_axpby (b_dev may be y_dev; it is not read when beta == 0) */
int pnl_gemv_multi(pnl_context *ctx, int m, const double *const *A_dev, int64_t ldA, int nrows, int ncols, const double *coeffs_host,
                   const double *x_dev, double alpha, double beta, const double *b_dev, double *y_dev);

/* ---- products with a block of vectors (csrc/pnl_block.hip): LinearOperator.matvec_multi / dotMV / A * X for a 2-D X
 *      (base/PyNucleus_base/LinearOperator_{SCALAR}.pxi:23-26, 64-76, 120-121). --------------------------------------------------------
 * Vectors are stored one per row, the layout of pnl_potrs / pnl_getrs: vector v is X_dev[v*ldx .. v*ldx + ncols), its result
 * Y_dev[v*ldy .. v*ldy + nrows).  Any nvec >= 1; the vectors are processed in groups of at most 16, one pass over the matrix per group
 * (nvec = 17 costs two passes).  Both calls are asynchronous on the context's stream and allocate nothing per call beyond growing a
 * scratch buffer of the context once.
 *
 * pnl_gemv_block: Y[v][r] = alpha * sum_c A[r][c] X[v][c] + beta * B[v][r], v < nvec, r < nrows; A row-major nrows x ncols (square or
 * rectangular), ldA >= ncols.  The contraction runs on v_mfma_f64_16x16x4_f64, a group of vectors being the 16-wide B operand (vectors
 * that do not exist are zero operands whose results are not stored).  No floating-point atomics: every reduction has a fixed shape
 * that depends on (nrows, ncols, ldA, alignment) only (more than 2048 columns are split over workgroups, whose partial sums go
 * through a scratch buffer of the context and are added in ascending order), so the same input gives the same bits, and the bits of
 * Y[v] depend neither on nvec nor on the position v nor on the other vectors.  beta == 0: B_dev may be NULL and is not read, Y is
 * overwritten (a NaN in Y before the call does not survive).  B_dev may equal Y_dev (with ldb == ldy); X must not overlap Y.
 * Unaligned bases, odd ldA and ld > n are correct (16-byte loads where the addresses allow, scalar loads otherwise); the padding
 * columns of A, X, B and Y are neither read into a sum nor written.  A symmetric matrix is read in full (no half-read as
 * pnl_gemv's symmetric_half = 2).  PNL_ERR_INVALID, before any launch, for a null ctx, A, X or Y; nvec, nrows or ncols < 1;
 * ldA < ncols, ldx < ncols or ldy < nrows; beta != 0 with a null B or ldb < nrows; X_dev == Y_dev. */
int pnl_gemv_block(pnl_context *ctx, const double *A_dev, int64_t ldA, int nrows, int ncols, int nvec, const double *X_dev, int64_t ldx,
                   double alpha, double beta, const double *B_dev, int64_t ldb, double *Y_dev, int64_t ldy);
/* The pattern resident in the context (pnl_upload_sparsity*), as pnl_spmv: CSR (diag_dev NULL) Y[v] = A X[v]; SSS (diag_dev given, data =
 * strict lower triangle) Y[v] = (L + L^T + D) X[v].  State and validation as pnl_spmv (PNL_ERR_STATE without a pattern, null data with
 * nnz > 0 invalid); nvec < 1, ldx or ldy below the number of DoFs and X_dev == Y_dev are invalid too.  Every (index, value) pair of the
 * matrix is loaded once per group of at most 16 vectors; the group is transposed once into a scratch buffer of the context.  CSR uses
 * no atomics and its bits are independent of nvec and of the position; SSS adds the mirrored entries with atomics (Y is zeroed by the
 * call): its contract is the value, not the bits. */
int pnl_spmv_block(pnl_context *ctx, const double *data_dev, const double *diag_dev, int nvec, const double *X_dev, int64_t ldx,
                   double *Y_dev, int64_t ldy);

/* ---- Jacobi-preconditioned CG for a block of right-hand sides (csrc/pnl_cg_block.hip): cg_solver.solve + jacobi_solver
 *      (base/PyNucleus_base/solvers.pyx:363-444, 229-245) for A X = B with several right-hand sides at once. --------------------------
 * Up to PNL_CGB_MAXVEC = 16 right-hand sides ("columns", stored one per row as in pnl_gemv_block) are solved together.  Every column
 * runs its OWN recurrence of pnl_cg_jacobi (its own alpha, beta and convergence; not a block Krylov method) and the columns share the
 * operator product, one pass over the operator per iteration.  The loop is that of pnl_cg_jacobi: update order x, r, (refresh),
 * z = D^-1 r, beta, p; a column has converged when sqrt(r . D^-1 r) <= tol (absolute); the residual is recomputed from b - A x when
 * the counter reaches 50, for every active column of the group at once; a column that converges in the first pass of the loop reports
 * 0 iterations, one that never converges reports maxiter.  A column that has converged is FROZEN: its x, r and reported residual are
 * no longer written.  A column whose r . D^-1 r is 0 at the start (b = 0 with x0 = 0) is frozen at once, with 0 iterations and
 * residual 0.  More than 16 columns are taken as consecutive groups of 16, each with a loop of its own.
 * No floating-point atomics: every dot product is summed in a shape that depends on n only.  With a product whose bits are independent
 * per vector (pnl_gemv_block; pnl_spmv_block on CSR; pnl_h2_matvec_block) the bits of X[v], iters[v] and residuals[v] depend neither
 * on the number of columns nor on the position v nor on the other columns, and two calls repeat bit for bit.  The scalars stay on the
 * device; the host reads the state of the group back once per iteration.  Nothing is allocated per call beyond growing buffers of the
 * context once.  The padding of B and X (ld > n) is neither read into a sum nor written.
 *
 * pnl_cg_jacobi_block: A dense, symmetric positive definite, row-major n x n, read in full by pnl_gemv_block (no half-read as
 * pnl_cg_jacobi).  X_dev holds the initial guesses and the results; iters[nrhs] and residuals[nrhs] on the host (either may be NULL).
 * Synchronous.  PNL_ERR_INVALID, before any launch, for a null ctx, A, B or X; n or nrhs < 1; ldA, ldb or ldx < n; maxiter < 0;
 * B_dev == X_dev. */
#define PNL_CGB_MAXVEC 16
int pnl_cg_jacobi_block(pnl_context *ctx, const double *A_dev, int64_t ldA, int n, int nrhs, const double *B_dev, int64_t ldb, double *X_dev,
                        int64_t ldx, double tol, int maxiter, int *iters, double *residuals);
/* The steps of that loop on caller-owned device blocks [nvec][ld], nvec <= 16, for operators whose product is not a dense block
 * (pnl_cg_jacobi_block is these calls around pnl_gemv_block).  dinv_dev: 1 / diagonal, n doubles; NULL: the unit diagonal (no
 * preconditioner).  state_dev: PNL_CGB_STATE doubles per column, column v at state_dev[v * PNL_CGB_STATE]:
 *   [0] betaOld = r . z of the pass before   [1] p . Ap   [2] beta = r . z   [3] conv = sqrt(beta)   [4] active (1 or 0)   [5 .. 7] 0
 *   pnl_cgb_init       R = B - AX (AX_dev NULL: X is zero, R = B), P = dinv R, betaOld = beta = R . P, conv, active = conv > tol and
 *                      beta != 0; writes the whole state of the columns v < nvec
 *   pnl_cgb_update     active columns: alpha = betaOld / (P . AP); X += alpha P; R -= alpha AP; Z = dinv R; beta = R . Z; conv
 *   pnl_cgb_refresh    active columns: R = B - AX, Z = dinv R, beta = R . Z, conv      (the recomputation every 50 iterations)
 *   pnl_cgb_direction  active columns: conv <= tol: active = 0, nothing else is written; else P = Z + (beta / betaOld) P, betaOld = beta
 * A pass of the loop is: AP = A P; update; every 50th pass AX = A X and refresh; direction; read the state.  Columns that are not
 * active are neither read nor written.  Asynchronous on the context's stream.  PNL_ERR_INVALID, before any launch, for a null
 * pointer (but dinv_dev, and AX_dev in pnl_cgb_init), n < 1, nvec < 1, nvec > 16, a leading dimension below n, two blocks that are
 * written or read and written being the same. */
#define PNL_CGB_STATE 8
int pnl_cgb_init(pnl_context *ctx, int n, int nvec, const double *dinv_dev, const double *B_dev, int64_t ldb, const double *AX_dev, int64_t ldax,
                 double *R_dev, int64_t ldr, double *P_dev, int64_t ldp, double tol, double *state_dev);
int pnl_cgb_update(pnl_context *ctx, int n, int nvec, const double *dinv_dev, const double *P_dev, int64_t ldp, const double *AP_dev, int64_t ldap,
                   double *X_dev, int64_t ldx, double *R_dev, int64_t ldr, double *Z_dev, int64_t ldz, double *state_dev);
int pnl_cgb_refresh(pnl_context *ctx, int n, int nvec, const double *dinv_dev, const double *B_dev, int64_t ldb, const double *AX_dev, int64_t ldax,
                    double *R_dev, int64_t ldr, double *Z_dev, int64_t ldz, double *state_dev);
int pnl_cgb_direction(pnl_context *ctx, int n, int nvec, const double *Z_dev, int64_t ldz, double *P_dev, int64_t ldp, double tol,
                      double *state_dev);
/* The same loop for a preconditioner that the caller applies between the steps, Z = M^-1 R on whole blocks (a multigrid cycle:
 * pnl_mg_cg_block is these calls around pnl_gemv_block and pnl_mg_cycle_block).  Blocks, state, partial sums, grid rule and validation
 * as above; the convergence measure is conv = sqrt(|R . Z|), as pnl_mg_cg takes it:
 *   pnl_cgb_residual   R = B - AX (AX_dev NULL: R = B).  state_dev NULL: every column v < nvec (the start, before there is a state);
 *                      else the active columns (the recomputation every 50 iterations).  The state is only read.
 *   pnl_cgb_start      with Z = M^-1 R of every column: P = Z, betaOld = beta = R . Z, conv, active = conv > tol and beta != 0; writes the
 *                      whole state of the columns v < nvec
 *   pnl_cgb_step       active columns: alpha = betaOld / (P . AP) (p . Ap goes to slot [1]); X += alpha P; R -= alpha AP
 *   pnl_cgb_beta       active columns, with Z = M^-1 R: beta = R . Z; conv = sqrt(|beta|)
 *   pnl_cgb_direction  as above
 * A pass of the loop is: AP = A P; step; every 50th pass AX = A X and residual; Z = M^-1 R; beta; direction; read the state.  The
 * preconditioner may run on every column: the Z of a column that is not active is not read.  Columns that are not active are neither
 * read nor written by these calls.  Asynchronous on the context's stream. */
int pnl_cgb_residual(pnl_context *ctx, int n, int nvec, const double *B_dev, int64_t ldb, const double *AX_dev, int64_t ldax, double *R_dev,
                     int64_t ldr, const double *state_dev);
int pnl_cgb_start(pnl_context *ctx, int n, int nvec, const double *R_dev, int64_t ldr, const double *Z_dev, int64_t ldz, double *P_dev, int64_t ldp,
                  double tol, double *state_dev);
int pnl_cgb_step(pnl_context *ctx, int n, int nvec, const double *P_dev, int64_t ldp, const double *AP_dev, int64_t ldap, double *X_dev, int64_t ldx,
                 double *R_dev, int64_t ldr, double *state_dev);
int pnl_cgb_beta(pnl_context *ctx, int n, int nvec, const double *R_dev, int64_t ldr, const double *Z_dev, int64_t ldz, double *state_dev);

/* ---- BiCGStab for a block of right-hand sides (csrc/pnl_bicgstab_block.hip): bicgstab_solver.solve
 *      (base/PyNucleus_base/solvers.pyx:716-787) for A X = B with a general (non-symmetric) A and several right-hand sides at once. ----
 * Up to PNL_CGB_MAXVEC = 16 right-hand sides ("columns", stored one per row as in pnl_gemv_block) are solved together.  Every column
 * runs its OWN recurrence of the reference's right-preconditioned BiCGStab (its own alpha, omega, beta, convergence and breakdown) and
 * the columns share the two operator products of a pass:
 *   start:  R = B - A X;  P = R;  R0 = M^-1 R;  P2 = M^-1 P;  kappa = R . R0;  res = sqrt(|kappa|)
 *   pass:   T = A P2;  alpha = kappa / (T . R0);  S = R - alpha T;  S2 = M^-1 S;  T2 = A S2;  omega = (T2 . S) / (T2 . T2);
 *           X += alpha P2 + omega S2;  R = S - omega T2;  res = sqrt(R . R);  kappaNew = R . R0;  res < tol: converged; else
 *           beta = kappaNew / kappa * alpha / omega;  P = R + beta (P - omega T);  P2 = M^-1 P;  kappa = kappaNew
 * Convergence is ||r||_2 < tol, absolute and strict, as in the reference; there is no test at the start and the residual is never
 * recomputed from b - A x.  A column that converges in the first pass reports 0 iterations, one that never converges maxiter.
 * maxiter = 0 returns res = sqrt(|kappa|) and leaves X alone.  A column that has converged is FROZEN: none of its blocks and nothing
 * of its state is written again.  More than 16 columns are taken as consecutive groups of 16, each with a loop of its own.
 * Breakdowns (the reference divides and returns NaN):
 *   kappa == 0 at the start (b = 0 with x0 = 0): frozen at once, 0 iterations, residual 0.
 *   T2 . T2 == 0 (S = 0, the lucky breakdown): omega := 0, so X += alpha P2, R = S, and the column converges by the normal test.
 *   A column whose next scalar would be 0 / 0, x / 0 or not finite -- T . R0 == 0; omega == 0 or kappaNew == 0 when the column has not
 *   converged; any sum that is not finite -- is frozen BEFORE a value that is not finite is written to one of its blocks.  Its
 *   iteration count is the pass in which this happened, its residual the last one computed: iterations < maxiter with
 *   residual >= tol identifies a breakdown.  The code stays in slot [6] of the state.
 * No floating-point atomics: every dot product is summed in a shape that depends on n only (that of the pnl_cgb_* steps).  With a
 * product whose bits are independent per vector (pnl_gemv_block; pnl_spmv_block on CSR; the ordered H2 far field) the bits of X[v],
 * iters[v] and residuals[v] depend neither on the number of columns nor on the position v nor on the other columns, and two calls
 * repeat bit for bit.  The padding of the blocks (ld > n) is neither read into a sum nor written.
 *
 * pnl_bicgstab_block: A dense, square, general, row-major n x n, read in full by pnl_gemv_block; nothing assumes symmetry.
 * jacobi != 0: M^-1 = 1 / diagonal (pnl_inv_diagonal); else M = I.  X_dev holds the initial guesses and the results; iters[nrhs] and
 * residuals[nrhs] on the host (either may be NULL).  Work comes from a growing buffer of the context; nothing else is allocated per
 * call.  Synchronous: the host reads the state of the group back once per pass.  PNL_ERR_INVALID, before any launch, for a null ctx,
 * A, B or X; n or nrhs < 1; ldA, ldb or ldx < n; maxiter < 0; B_dev == X_dev or A_dev == X_dev. */
int pnl_bicgstab_block(pnl_context *ctx, const double *A_dev, int64_t ldA, int n, int nrhs, int jacobi, const double *B_dev, int64_t ldb,
                       double *X_dev, int64_t ldx, double tol, int maxiter, int *iters, double *residuals);
/* The steps of that loop on caller-owned device blocks [nvec][ld], nvec <= 16 (pnl_bicgstab_block is exactly these calls around
 * pnl_gemv_block).  Preconditioner: external == 0: M^-1 = dinv_dev (1 / diagonal, n doubles; NULL: the unit diagonal), applied by the
 * steps; external != 0: the caller applies M^-1 on whole blocks between the calls, the steps neither read dinv_dev nor touch R0 (init),
 * S2 (alpha) or P2 (init, direction), which may then be NULL.  state_dev: PNL_BCGB_STATE doubles per column, column v at
 * state_dev[v * PNL_BCGB_STATE]:
 *   [0] kappa   [1] alpha   [2] omega   [3] res   [4] active (1 or 0)   [5] kappaNew = R . R0   [6] breakdown code PNL_BCGB_*
 *   [7] T . R0   [8] T2 . S   [9] T2 . T2   [10] R . R   [11] beta
 *   pnl_bcgb_init       every column: R = B - AX (AX_dev NULL: X is zero, R = B), P = R; external == 0: also R0 = P2 = dinv R and the
 *                       start state as pnl_bcgb_start
 *   pnl_bcgb_start      with the caller's R0 = M^-1 R of every column: kappa = R . R0, res = sqrt(|kappa|), active = kappa is finite
 *                       and not 0; writes the whole state of the columns v < nvec.  (The caller also sets P2 = R0.)
 *   pnl_bcgb_alpha      active columns: alpha = kappa / (T . R0); S = R - alpha T, written over R (RS_dev); external == 0: S2 = dinv S.
 *                       T . R0 == 0 or not finite: the code is set and none of the column's blocks is written
 *   pnl_bcgb_omega      live columns (active, no code): omega; X += alpha P2 + omega S2; R = S - omega T2 over S (RS_dev); res,
 *                       kappaNew; then res < tol: active = 0; a breakdown: the code and active = 0; else beta and kappa = kappaNew.
 *                       Clears active of a column whose code pnl_bcgb_alpha has set; its res stays
 *   pnl_bcgb_direction  active columns: P = R + beta (P - omega T); external == 0: P2 = dinv P.  The state is only read
 * A pass of the loop is: T = A P2; alpha; (S2 = M^-1 S); T2 = A S2; omega; direction; (P2 = M^-1 P); read the state.  Columns that are
 * not active are neither read nor written.  Asynchronous on the context's stream.  PNL_ERR_INVALID, before any launch, for a null
 * pointer (but dinv_dev, AX_dev in pnl_bcgb_init and the blocks an external preconditioner owns), n < 1, nvec < 1, nvec > 16, a
 * leading dimension below n, a block that is written being the same as another block of the call. */
#define PNL_BCGB_STATE 12
#define PNL_BCGB_OK 0
#define PNL_BCGB_TR0 1          /* T . R0 == 0 */
#define PNL_BCGB_OMEGA 2        /* omega == 0 and the column has not converged */
#define PNL_BCGB_KAPPA 3        /* kappaNew == 0 and the column has not converged */
#define PNL_BCGB_NONFINITE 4    /* a sum or a scalar that is not finite */
int pnl_bcgb_init(pnl_context *ctx, int n, int nvec, int external, const double *dinv_dev, const double *B_dev, int64_t ldb, const double *AX_dev,
                  int64_t ldax, double *R_dev, int64_t ldr, double *P_dev, int64_t ldp, double *R0_dev, int64_t ldr0, double *P2_dev, int64_t ldp2,
                  double *state_dev);
int pnl_bcgb_start(pnl_context *ctx, int n, int nvec, const double *R_dev, int64_t ldr, const double *R0_dev, int64_t ldr0, double *state_dev);
int pnl_bcgb_alpha(pnl_context *ctx, int n, int nvec, int external, const double *dinv_dev, const double *T_dev, int64_t ldt, const double *R0_dev,
                   int64_t ldr0, double *RS_dev, int64_t ldr, double *S2_dev, int64_t lds2, double *state_dev);
int pnl_bcgb_omega(pnl_context *ctx, int n, int nvec, const double *P2_dev, int64_t ldp2, const double *S2_dev, int64_t lds2, const double *T2_dev,
                   int64_t ldt2, const double *R0_dev, int64_t ldr0, double *X_dev, int64_t ldx, double *RS_dev, int64_t ldr, double tol,
                   double *state_dev);
int pnl_bcgb_direction(pnl_context *ctx, int n, int nvec, int external, const double *dinv_dev, const double *R_dev, int64_t ldr, const double *T_dev,
                       int64_t ldt, double *P_dev, int64_t ldp, double *P2_dev, int64_t ldp2, const double *state_dev);

/* ---- multigrid for a block of right-hand sides (csrc/pnl_mg_block.hip): the cycle of pnl_mg_cycle and the loop of pnl_mg_cg for several
 *      right-hand sides on one hierarchy. -----------------------------------------------------------------------------------------------
 * Columns are stored one per row as in pnl_gemv_block: column v is B_dev[v*ldb .. v*ldb + n), its result X_dev[v*ldx .. v*ldx + n), n the
 * size of the finest level.  The columns are processed in groups of at most 16; a group shares every pass over an operator.  Every level
 * of the hierarchy must be dense (kind 0 or 2; both are read in full by pnl_gemv_block, no half-read of a symmetric level): a hierarchy
 * whose finest level is an H2 operator (kind 1) is refused with PNL_ERR_INVALID.  The level blocks ([16][n_l] for rhs, sol and temp) are
 * allocated by the first block call on the hierarchy, not by pnl_mg_create.  No floating-point atomics: the residuals and the coarse solve
 * are pnl_gemv_block launches, the damped-Jacobi update and the transfer operators give one thread one row of the block and loop over the
 * columns (sums in ascending order of the stored entries), the dot products are those of the pnl_cgb_* steps.  The bits of column v --
 * X[v], iters[v], residuals[v] -- therefore depend neither on the number of columns nor on the position v nor on the other columns, and
 * two calls repeat bit for bit.  They are not the bits of pnl_mg_cycle / pnl_mg_cg, which sum in another order.  The padding of B and X
 * (ld > n) is neither read into a sum nor written.
 *
 * pnl_mg_cycle_block: one V cycle (solveOnLevel) on the finest level for nvec >= 1 columns.  x_is_zero: X counts as zero whatever it
 * holds (it is not read), the first residual is B; else X holds the iterates.  Asynchronous on the context's stream, no host
 * synchronisation inside.  PNL_ERR_INVALID, before any launch, for a null mg, B or X; nvec < 1; ldb or ldx < n; B_dev == X_dev; an H2
 * finest level.
 *
 * pnl_mg_cg_block: pnl_mg_cg for nrhs columns; A_dev NULL: the finest operator of the hierarchy, else a dense row-major n x n operator
 * (symmetric positive definite, read in full).  Every column runs the recurrence of pnl_mg_cg on its OWN (its own alpha, beta and
 * convergence on sqrt(|r . M^-1 r|) <= tol, M^-1 = one V cycle from a zero guess); per iteration and group the columns share one
 * pnl_gemv_block for A P and one pnl_mg_cycle_block for Z.  A column that has converged is FROZEN (its x, r and reported residual are no
 * longer written; the cycle still carries it along), one whose r . M^-1 r is 0 at the start is frozen at once with 0 iterations and
 * residual 0.  Iteration counts as pnl_mg_cg: a column that converges in the first pass reports 0, one that never converges maxiter.
 * The residual is recomputed from b - A x when the counter reaches 50, for the active columns of the group.  More than 16 columns are
 * taken as consecutive groups, each with a loop of its own.  x_is_zero: the caller states that X holds zeros (as for pnl_mg_cg), R = B
 * without a product; else X holds the initial guesses.  maxiter = 0 leaves X untouched and reports the initial conv.  iters[nrhs] and
 * residuals[nrhs] (the final conv) on the host, either may be NULL.  Synchronous: the host reads the state of the group back once per
 * iteration.  PNL_ERR_INVALID, before any launch, for a null mg, B or X; nrhs < 1; ldb or ldx < n; ldA < n with a given A; maxiter < 0;
 * B_dev == X_dev; an H2 finest level. */
int pnl_mg_cycle_block(pnl_mg *mg, int nvec, const double *B_dev, int64_t ldb, double *X_dev, int64_t ldx, int x_is_zero);
int pnl_mg_cg_block(pnl_mg *mg, const double *A_dev, int64_t ldA, int nrhs, const double *B_dev, int64_t ldb, double *X_dev, int64_t ldx,
                    double tol, int maxiter, int x_is_zero, int *iters, double *residuals);

/* ---- the vector side of a block eigensolver (csrc/pnl_eig_block.hip): the three contractions of LOBPCG for the smallest eigenpairs of
 *      A x = lambda M x on blocks of vectors (solvers.lobpcg runs the loop; the small Rayleigh-Ritz problem stays on the host). ----------
 * Blocks are row-major [k][ld] with ld >= n, one vector per row as in pnl_gemv_block; padding columns are neither read into a sum nor
 * written.  Asynchronous on the context's stream.  No floating-point atomics: every sum has a shape that depends on n only (the grid
 * rule of the pnl_cgb_* steps: element i belongs to workgroup (i / 256) mod min(256, ceil(n / 256))), so the same input gives the
 * same bits.  PNL_ERR_INVALID, before any launch, for a null pointer (but dinv_dev and W_dev of pnl_eigb_residual), a size out of
 * range, a leading dimension below its row length, a written block that is also an input of the call.
 *
 * pnl_eigb_gram: G[a*ldg + b] = sum_i U[a][i] V[b][i], 1 <= ku, kv <= PNL_EIGB_MAXBASIS (three groups of 16 rows), ldg >= kv: the
 * Gram matrix of the Rayleigh-Ritz step.  v_mfma_f64_16x16x4_f64 with 16 rows of U as the A operand, 16 rows of V as the B operand
 * and the n direction as MFMA's k; rows that do not exist are zero operands whose results are not stored.  A workgroup writes its
 * 16 x 16 partial tiles to a scratch buffer of the context, a second launch adds them in ascending workgroup order.  The bits of
 * G[a][b] depend on U[a], V[b] and n only -- not on ku, kv, the positions a and b or the other rows; with U_dev == V_dev and
 * ldu == ldv G is bitwise symmetric.
 *
 * pnl_eigb_combine: Y[a][i] = sum_{b < kin} C[a*ldc + b] S[b][i], kin <= PNL_EIGB_MAXBASIS, kout <= 16, ldc >= kin, C in device
 * memory: the basis rotation X <- C^T [X; W; P].  Per element t = C[a][0] S[0][i], then t = fma(C[a][b], S[b][i], t) in ascending b;
 * every S[b][i] is loaded once per call.  Y must be neither S nor C.
 *
 * pnl_eigb_residual: for the columns v < nv <= 16 whose bit is set in mask (mask != 0, no bit at or above nv):
 * R_v = fma(-theta_v, MX_v, AX_v); W_v = dinv R_v where W_dev is given (dinv_dev NULL: the unit diagonal, W_v = R_v);
 * sums_dev[2 v] = R_v . R_v, sums_dev[2 v + 1] = MX_v . MX_v.  theta_dev: nv doubles, sums_dev: 2 nv doubles, both on the device.
 * Columns outside mask are neither read nor written (their sums neither).  AX_dev and MX_dev may be any two blocks that are only
 * read (MX_dev is the X block when M = I); R_dev and W_dev must differ from each other and from both. */
#define PNL_EIGB_MAXBASIS 48
int pnl_eigb_gram(pnl_context *ctx, int n, int ku, const double *U_dev, int64_t ldu, int kv, const double *V_dev, int64_t ldv, double *G_dev,
                  int64_t ldg);
int pnl_eigb_combine(pnl_context *ctx, int n, int kin, const double *S_dev, int64_t lds, int kout, const double *C_dev, int64_t ldc,
                     double *Y_dev, int64_t ldy);
int pnl_eigb_residual(pnl_context *ctx, int n, int nv, unsigned mask, const double *AX_dev, int64_t ldax, const double *MX_dev, int64_t ldmx,
                      const double *theta_dev, const double *dinv_dev, double *R_dev, int64_t ldr, double *W_dev, int64_t ldw,
                      double *sums_dev);

#ifdef __cplusplus
}
#endif
#endif
