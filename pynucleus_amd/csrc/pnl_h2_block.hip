// H2 far field for a block of up to 16 vectors, free of floating-point atomics (gfx950 only): pnl_h2_matvec_block and its three
// phases pnl_h2_upward_block / _interact_block / _downward_block, and the index structures pnl_h2_setup derives for them.
//
// The single-vector kernels of pnl_h2.hip take one wave per SOURCE (child, admissible pair) and merge the contributions of a node with
// atomics.  Here a workgroup belongs to a DESTINATION (leaf, parent, n1, child) and adds that node's sources in an order the plan
// fixes: a leaf its DoFs in ascending order, a parent its children in ascending node number, n1 its pairs in ascending pair index.
// Coefficient blocks are [nnodes][M][16], the vector index fastest; vectors are stored one per row as in pnl_gemv_block.
//
//   contraction  v_mfma_f64_16x16x4_f64: 16 rows of the M x M block (of T, K, or of V / V^T) are the A operand, the 16 vectors the B
//                operand; vectors that do not exist are zero operands whose results are stored as zero (coefficients) or not at all (Y).
//                Lane (m = l & 15, q = l >> 4) supplies for step pair j the columns 8 j + 2 q, + 1 of row r0 + m (one 16-byte load
//                where the address allows it -- M is odd more often than not --, two 8-byte loads otherwise: the same bits); MFMA
//                (j, h) contracts the four columns 8 j + 2 q + h, q = 0 .. 3.  The transposed blocks (T^T of the downward pass, V^T of
//                the leaves) are read as A[c][r]: the 16 m lanes then read 128 contiguous bytes.  D: lane (m, q) holds rows
//                q + 4 t of the tile, t = 0 .. 3, for vector m.
//   staging      the source coefficient block (M x 16, at most 32 KB) lies in LDS in operand order [j][h][q][v]: MFMA (j, h) reads 64
//                contiguous doubles (no bank conflict).  Columns between M and the next multiple of 8 are zero in LDS and are not
//                loaded from the block.  The leaves stage the gathered X[v][dofs] the same way, HB_KC DoFs at a time.
//   workgroup    4 waves; wave w owns the row tiles w, w + 4, w + 8, w + 12 (M <= 256) and keeps their accumulators in registers
//                across ALL sources of the destination: one chain of MFMAs per (row, vector), sources in plan order, columns in
//                ascending groups.  Rows beyond M read row M - 1 (rows of the A operand do not mix) and are not stored.
//   sums         no atomics, no partial sums across workgroups: the shape of every sum depends on the plan and on M only, and a column
//                of the B operand never enters another column's result.  The bits of Y[v] therefore do not depend on nvec, on v, on
//                the other vectors or on the call.
// The levels stay separate launches (the tree imposes the order); the interactions write every node's block (zero without pairs), so
// cdownB needs no fill.
#include "pnl_context.h"
#include "pnl_common.h"

namespace {

constexpr int HB_NV = 16;                  // vectors per group = columns of the MFMA's B operand
constexpr int HB_WAVES = 4;
constexpr int HB_THREADS = 64*HB_WAVES;
constexpr int HB_TI = 4;                   // row tiles per wave: 16 HB_WAVES HB_TI = 256 rows
constexpr int HB_KC = 256;                 // contraction columns per LDS stage (M <= HB_KC; the leaves take their DoFs in such chunks)
constexpr int HB_JG = 8;                   // step pairs (8 columns each) whose loads of the A operand are in flight together
constexpr int HB_MAXM = 16*HB_WAVES*HB_TI;
static_assert(HB_MAXM <= HB_KC && HB_KC % 8 == 0, "a coefficient block is one stage");

typedef double hb_d2 __attribute__((ext_vector_type(2)));
typedef double hb_d4 __attribute__((ext_vector_type(4)));

// LDS slot of (contraction column c, vector v): [j = c / 8][h = c & 1][q = (c / 2) & 3][v]
__device__ __forceinline__ int hb_slot(int c, int v) { return ((((c >> 3) << 1)+(c & 1)) << 6)+(((c >> 1) & 3) << 4)+v; }

// stage the coefficient block src[M][16]
__device__ __forceinline__ void hb_stage_block(const double *src, int M, double *sS) {
    const int n = ((M+7) & ~7)*HB_NV;
    for (int t = threadIdx.x; t < n; t += HB_THREADS) sS[hb_slot(t >> 4, t & 15)] = t < M*HB_NV ? src[t] : 0.;
}

// stage X[v][dofs[c]], c < kc <= HB_KC, v < nv; zero for the vectors that do not exist and up to the next multiple of 8 columns
__device__ __forceinline__ void hb_stage_x(const double *__restrict__ X, long long ldx, int nv, const int *__restrict__ dofs, int kc, double *sS) {
    const int kcp = (kc+7) & ~7;
    for (int t = threadIdx.x; t < kcp*HB_NV; t += HB_THREADS) {
        const int v = t/kcp, c = t-v*kcp;
        sS[hb_slot(c, v)] = (v < nv && c < kc) ? X[v*ldx+dofs[c]] : 0.;
    }
}

// acc += A(r0 + 4 t + q, c) S[c][m] over the staged columns c < kc.  !TRANS: A(r, c) = A[r ld + c]; TRANS: A(r, c) = A[c ld + r].
// R rows exist.  Uniform over the wave.
template <bool TRANS>
__device__ __forceinline__ void hb_tile(const double *__restrict__ A, int ld, int R, int r0, int kc, const double *sS, hb_d4 &acc) {
    const int lane = threadIdx.x & 63, m = lane & 15, q = lane >> 4;
    const int r = min(r0+m, R-1);
    const double *__restrict__ arow = TRANS ? A+r : A+(size_t)r*ld;
    // HB_JG step pairs (64 columns) at a time: their loads are all issued before the first MFMA waits for one
    for (int j0 = 0; 8*j0 < kc; j0 += HB_JG) {
        double a0[HB_JG], a1[HB_JG];
#pragma unroll
        for (int i = 0; i < HB_JG; i++) {
            const int c = 8*(j0+i)+2*q;
            a0[i] = 0.; a1[i] = 0.;
            if (TRANS) {
                if (c < kc) a0[i] = arow[(size_t)c*ld];
                if (c+1 < kc) a1[i] = arow[(size_t)(c+1)*ld];
            } else {
                const double *p = arow+c;
                if (c+1 < kc && (((uintptr_t)p) & 15) == 0) {
                    const hb_d2 t = *(const hb_d2*)p;
                    a0[i] = t.x; a1[i] = t.y;
                } else {
                    if (c < kc) a0[i] = p[0];
                    if (c+1 < kc) a1[i] = p[1];
                }
            }
        }
#pragma unroll
        for (int i = 0; i < HB_JG; i++) {
            const int j = j0+i;
            if (8*j < kc) {                       // uniform over the wave
                const double b0 = sS[((2*j) << 6)+lane], b1 = sS[((2*j+1) << 6)+lane];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a0[i], b0, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a1[i], b1, acc, 0, 0, 0);
            }
        }
    }
}

// upward pass, leaves: cupB[node][alpha][v] = sum_k X[v][dofs[k]] V[k][alpha], k ascending; 0 for v >= nv
__global__ void __launch_bounds__(HB_THREADS)
k_h2b_up_leaves(const H2Dev H, const double *__restrict__ X, long long ldx, int nv, double *__restrict__ cupB) {
    __shared__ double sS[HB_KC*HB_NV];
    const int lf = blockIdx.x, node = H.leaf_node[lf], M = H.M;
    const int *dofs = H.leaf_dofs+H.leaf_dof_off[lf];
    const int nd = H.leaf_dof_off[lf+1]-H.leaf_dof_off[lf];
    const double *V = H.V+H.leaf_val_off[lf];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m = lane & 15, q = lane >> 4;
    hb_d4 acc[HB_TI];
#pragma unroll
    for (int ti = 0; ti < HB_TI; ti++) acc[ti] = (hb_d4){0., 0., 0., 0.};
    for (int k0 = 0; k0 < nd; k0 += HB_KC) {
        const int kc = min(HB_KC, nd-k0);
        hb_stage_x(X, ldx, nv, dofs+k0, kc, sS);
        __syncthreads();
#pragma unroll
        for (int ti = 0; ti < HB_TI; ti++) {
            const int r0 = 16*(wv+HB_WAVES*ti);
            if (r0 < M) hb_tile<true>(V+(size_t)k0*M, M, M, r0, kc, sS, acc[ti]);
        }
        __syncthreads();
    }
    double *out = cupB+(size_t)node*M*HB_NV;
#pragma unroll
    for (int ti = 0; ti < HB_TI; ti++)
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int row = 16*(wv+HB_WAVES*ti)+q+4*t;
            if (row < M) out[row*HB_NV+m] = m < nv ? acc[ti][t] : 0.;
        }
}

// one workgroup per destination node, its sources in the order of the lists:
//   MODE 0  upward level:   dst[p] += T_c src[c]        over the children c = idx[ptr[p] ..] of the parent p = nodes[block] (src = dst = cupB)
//   MODE 1  interactions:   dst[n1] = sum K_pr src[n2]  over the pairs pr = idx[ptr[n1] ..] of n1 = block (every node; src = cupB, dst = cdownB)
//   MODE 2  downward level: dst[c] += T_c^T src[parent] for the child c = nodes[block] (src = dst = cdownB; the parent's level is finished)
template <int MODE>
__global__ void __launch_bounds__(HB_THREADS)
k_h2b_nodes(const H2Dev H, const int *__restrict__ nodes, const int *__restrict__ ptr, const int *__restrict__ idx, const double *src, double *dst) {
    __shared__ double sS[HB_KC*HB_NV];
    const int M = H.M, dest = MODE == 1 ? (int)blockIdx.x : nodes[blockIdx.x];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m = lane & 15, q = lane >> 4;
    double *out = dst+(size_t)dest*M*HB_NV;
    hb_d4 acc[HB_TI];
#pragma unroll
    for (int ti = 0; ti < HB_TI; ti++)
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int row = 16*(wv+HB_WAVES*ti)+q+4*t;
            acc[ti][t] = (MODE != 1 && row < M) ? out[row*HB_NV+m] : 0.;
        }
    const int eb = MODE == 2 ? 0 : ptr[dest], ee = MODE == 2 ? 1 : ptr[dest+1];
    for (int e = eb; e < ee; e++) {
        int sn;
        const double *B;
        if (MODE == 0) { sn = idx[e]; B = H.T+(size_t)sn*M*M; }
        else if (MODE == 1) { const int pr = idx[e]; sn = H.far[2*pr+1]; B = H.K+(size_t)pr*M*M; }
        else { sn = H.parent[dest]; B = H.T+(size_t)dest*M*M; }
        hb_stage_block(src+(size_t)sn*M*HB_NV, M, sS);
        __syncthreads();
#pragma unroll
        for (int ti = 0; ti < HB_TI; ti++) {
            const int r0 = 16*(wv+HB_WAVES*ti);
            if (r0 < M) hb_tile<MODE == 2>(B, M, M, r0, M, sS, acc[ti]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int ti = 0; ti < HB_TI; ti++)
#pragma unroll
        for (int t = 0; t < 4; t++) {
            const int row = 16*(wv+HB_WAVES*ti)+q+4*t;
            if (row < M) out[row*HB_NV+m] = acc[ti][t];
        }
}

// downward pass, leaves: Y[v][dofs[k]] += sum_alpha V[k][alpha] cdownB[node][alpha][v], v < nv (the leaves are disjoint: one writer per DoF)
__global__ void __launch_bounds__(HB_THREADS)
k_h2b_down_leaves(const H2Dev H, const double *__restrict__ cdownB, int nv, double *__restrict__ Y, long long ldy) {
    __shared__ double sS[HB_KC*HB_NV];
    const int lf = blockIdx.x, node = H.leaf_node[lf], M = H.M;
    const int *dofs = H.leaf_dofs+H.leaf_dof_off[lf];
    const int nd = H.leaf_dof_off[lf+1]-H.leaf_dof_off[lf];
    if (nd == 0) return;
    const double *V = H.V+H.leaf_val_off[lf];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, m = lane & 15, q = lane >> 4;
    hb_stage_block(cdownB+(size_t)node*M*HB_NV, M, sS);
    __syncthreads();
    for (int r0 = 16*wv; r0 < nd; r0 += 16*HB_WAVES) {
        hb_d4 acc = (hb_d4){0., 0., 0., 0.};
        hb_tile<false>(V, M, nd, r0, M, sS, acc);
        if (m < nv) {
#pragma unroll
            for (int t = 0; t < 4; t++) {
                const int k = r0+q+4*t;
                if (k < nd) Y[m*ldy+dofs[k]] += acc[t];
            }
        }
    }
}

// state and sizes of a block call: PNL_ERR_INVALID for null arguments is the caller's
int hb_ready(pnl_context *ctx, const char *who, int nvec, bool phase) {
    if (!ctx->have_h2) return fail(ctx, PNL_ERR_STATE, "pnl_h2_setup first");
    if (nvec < 1 || (phase && nvec > HB_NV)) return fail(ctx, PNL_ERR_INVALID, "%s: nvec = %d (1 .. 16 in the phase calls)", who, nvec);
    if (ctx->h2.M > HB_MAXM) return fail(ctx, PNL_ERR_UNSUPPORTED, "%s: M = %d > %d", who, ctx->h2.M, HB_MAXM);
    return PNL_OK;
}

int hb_upward(pnl_context *ctx, int nv, const double *X, long long ldx, double *cupB) {
    const H2Dev &H = ctx->h2;
    const int *par = (const int*)ctx->b_h2[24].p, *cptr = (const int*)ctx->b_h2[22].p, *cidx = (const int*)ctx->b_h2[23].p;
    HIPCHK(ctx, hipMemsetAsync(cupB, 0, sizeof(double)*(size_t)H.nnodes*H.M*HB_NV, ctx->stream));
    hipLaunchKernelGGL(k_h2b_up_leaves, dim3(H.nleaves), dim3(HB_THREADS), 0, ctx->stream, H, X, ldx, nv, cupB);
    for (int l = (int)ctx->h2_par_off.size()-2; l >= 0; l--) {
        const int n = (int)(ctx->h2_par_off[l+1]-ctx->h2_par_off[l]);
        if (n) hipLaunchKernelGGL((k_h2b_nodes<0>), dim3(n), dim3(HB_THREADS), 0, ctx->stream, H, par+ctx->h2_par_off[l], cptr, cidx, (const double*)cupB, cupB);
    }
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

int hb_interact(pnl_context *ctx, const double *cupB, double *cdownB) {
    const H2Dev &H = ctx->h2;
    hipLaunchKernelGGL((k_h2b_nodes<1>), dim3(H.nnodes), dim3(HB_THREADS), 0, ctx->stream, H, (const int*)nullptr, (const int*)ctx->b_h2[20].p,
                       (const int*)ctx->b_h2[21].p, cupB, cdownB);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

int hb_downward(pnl_context *ctx, int nv, double *cdownB, double *Y, long long ldy) {
    const H2Dev &H = ctx->h2;
    const int nlev = (int)ctx->h2_levels.size();
    const int *lev = (const int*)ctx->b_h2[17].p;
    for (int l = 1; l < nlev; l++) {
        const int n = (int)ctx->h2_levels[l].size();
        if (n) hipLaunchKernelGGL((k_h2b_nodes<2>), dim3(n), dim3(HB_THREADS), 0, ctx->stream, H, lev+ctx->h2_level_off[l], (const int*)nullptr,
                                  (const int*)nullptr, (const double*)cdownB, cdownB);
    }
    hipLaunchKernelGGL(k_h2b_down_leaves, dim3(H.nleaves), dim3(HB_THREADS), 0, ctx->stream, H, (const double*)cdownB, nv, Y, ldy);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

}  // namespace

// for pnl_h2_setup, once the plan is validated: the pairs of every n1 in ascending pair index (b_h2[20], [21]), the children of every node
// in ascending node number (b_h2[22], [23]) and the parents of every level (b_h2[24], h2_par_off)
int pnl_h2_block_plan(pnl_context *ctx, const pnl_h2_plan *pl) {
    const int nn = pl->nnodes;
    std::vector<int> fptr(nn+1, 0), fidx(std::max(pl->nfar, 1)), cptr(nn+1, 0), cidx(nn);
    for (int p = 0; p < pl->nfar; p++) fptr[pl->far[2*p]+1]++;
    for (int n = 0; n < nn; n++) {
        fptr[n+1] += fptr[n];
        if (pl->parent[n] >= 0) cptr[pl->parent[n]+1]++;
    }
    for (int n = 0; n < nn; n++) cptr[n+1] += cptr[n];
    std::vector<int> ffill(fptr.begin(), fptr.end()-1), cfill(cptr.begin(), cptr.end()-1);
    for (int p = 0; p < pl->nfar; p++) fidx[ffill[pl->far[2*p]]++] = p;
    for (int n = 0; n < nn; n++)
        if (pl->parent[n] >= 0) cidx[cfill[pl->parent[n]]++] = n;
    std::vector<int> par;
    ctx->h2_par_off.assign(pl->nlevels+1, 0);
    for (int l = 0; l < pl->nlevels; l++) {
        ctx->h2_par_off[l] = par.size();
        for (int n = 0; n < nn; n++)
            if (pl->level[n] == l && cptr[n+1] > cptr[n]) par.push_back(n);
    }
    ctx->h2_par_off[pl->nlevels] = par.size();
    int rc;
    DevBuf *B = ctx->b_h2;
    if ((rc = upload(ctx, B[20], fptr.data(), fptr.size())) || (rc = upload(ctx, B[21], fidx.data(), (size_t)pl->nfar)) ||
        (rc = upload(ctx, B[22], cptr.data(), cptr.size())) || (rc = upload(ctx, B[23], cidx.data(), cidx.size())) ||
        (rc = upload(ctx, B[24], par.data(), par.size())))
        return rc;
    return PNL_OK;
}

extern "C" {

int pnl_h2_upward_block(pnl_context *ctx, int nvec, const double *X_dev, int64_t ldx, double *cupB_dev) {
    if (!ctx || !X_dev || !cupB_dev) return PNL_ERR_INVALID;
    if (int rc = hb_ready(ctx, "pnl_h2_upward_block", nvec, true)) return rc;
    if (ldx < ctx->N) return fail(ctx, PNL_ERR_INVALID, "pnl_h2_upward_block: ldx = %lld < %d", (long long)ldx, ctx->N);
    return hb_upward(ctx, nvec, X_dev, (long long)ldx, cupB_dev);
}

int pnl_h2_interact_block(pnl_context *ctx, const double *cupB_dev, double *cdownB_dev) {
    if (!ctx || !cupB_dev || !cdownB_dev || cupB_dev == cdownB_dev) return PNL_ERR_INVALID;
    if (int rc = hb_ready(ctx, "pnl_h2_interact_block", 1, true)) return rc;
    return hb_interact(ctx, cupB_dev, cdownB_dev);
}

int pnl_h2_downward_block(pnl_context *ctx, int nvec, double *cdownB_dev, double *Y_dev, int64_t ldy) {
    if (!ctx || !cdownB_dev || !Y_dev) return PNL_ERR_INVALID;
    if (int rc = hb_ready(ctx, "pnl_h2_downward_block", nvec, true)) return rc;
    if (ldy < ctx->N) return fail(ctx, PNL_ERR_INVALID, "pnl_h2_downward_block: ldy = %lld < %d", (long long)ldy, ctx->N);
    return hb_downward(ctx, nvec, cdownB_dev, Y_dev, (long long)ldy);
}

int pnl_h2_matvec_block(pnl_context *ctx, int nvec, const double *X_dev, int64_t ldx, double *Y_dev, int64_t ldy) {
    if (!ctx || !X_dev || !Y_dev) return PNL_ERR_INVALID;
    if (int rc = hb_ready(ctx, "pnl_h2_matvec_block", nvec, false)) return rc;
    if (ldx < ctx->N || ldy < ctx->N || X_dev == Y_dev)
        return fail(ctx, PNL_ERR_INVALID, "pnl_h2_matvec_block: bad arguments (ldx=%lld ldy=%lld n=%d)", (long long)ldx, (long long)ldy, ctx->N);
    const size_t bytes = sizeof(double)*(size_t)ctx->h2.nnodes*ctx->h2.M*HB_NV;
    int rc;
    if ((rc = ensure(ctx, ctx->b_h2[25], bytes)) || (rc = ensure(ctx, ctx->b_h2[26], bytes))) return rc;
    double *cupB = (double*)ctx->b_h2[25].p, *cdownB = (double*)ctx->b_h2[26].p;
    for (int v0 = 0; v0 < nvec; v0 += HB_NV) {
        const int nv = std::min(HB_NV, nvec-v0);
        if ((rc = hb_upward(ctx, nv, X_dev+(long long)v0*ldx, (long long)ldx, cupB)) || (rc = hb_interact(ctx, cupB, cdownB)) ||
            (rc = hb_downward(ctx, nv, cdownB, Y_dev+(long long)v0*ldy, (long long)ldy)))
            return rc;
    }
    return PNL_OK;
}

}  // extern "C"
