// H2 far field of the nonlocal operators (gfx950 only): kernels and host code of pnl_h2_setup, pnl_h2_matvec and its three phases,
// pnl_h2_get / _set / _sizes.  The atomic-free far field for blocks of vectors is pnl_h2_block.hip.  The near field of an H2 operator is assembled by pnl_hip.hip (pnl_assemble_clusters_tiled).
//
// Reference (clusterMethodCy.pyx): Chebyshev interpolation of the kernel on admissible cluster pairs
// (assembleFarFieldInteractions :2153-2238, factor -2 for the (u(x)-u(y))(v(x)-v(y)) form), leaf values
// int phi_I L_alpha (enterLeafValues :1205-1325), upward / downward passes with the transfer operators
// (:1092-1124, :1157-1180; the transfer matrices :2004-2073 are built on the host) and H2Matrix.matvec :2269-2295.
// Tensor index alpha = alpha_0 + m alpha_1 (coordinate 0 fastest) in every array of this file.
// struct H2Dev, cheb_node, lagrange1d: pnl_device.h; k_h2_kernel_interp_pw (order per quadrature point): pnl_pointwise.h
#include "pnl_context.h"
#include "pnl_common.h"
#include "pnl_dispatch.h"

template <int DIM>
__global__ void __launch_bounds__(PNL_NTHREADS)
k_h2_kernel_interp(const DevProblem P, const H2Dev H, const DevKernel *__restrict__ kcls, const int *__restrict__ far_class) {
    const int pr = blockIdx.x, n1 = H.far[2*pr], n2 = H.far[2*pr+1];
    const DevKernel kn = far_class ? kcls[far_class[pr]] : P.k;
    const double *b1 = H.box+(size_t)n1*DIM*2, *b2 = H.box+(size_t)n2*DIM*2;
    for (int t = threadIdx.x; t < H.M*H.M; t += PNL_NTHREADS) {
        const int i = t/H.M, j = t-i*H.M;
        double d2 = 0.;
        int ii = i, jj = j;
#pragma unroll
        for (int d = 0; d < DIM; d++) {
            const double x = cheb_node(b1[2*d], b1[2*d+1], H.m, ii % H.m), y = cheb_node(b2[2*d], b2[2*d+1], H.m, jj % H.m);
            ii /= H.m; jj /= H.m;
            d2 += (x-y)*(x-y);
        }
        H.K[(size_t)pr*H.M*H.M+t] = -2.*kern_eval<0>(kn, d2);
    }
}

// V_leaf[lcl_dof][alpha] = sum over the cells of the leaf and the quadrature points of vol w phi_k(x) L_alpha(x)
template <int DIM, int DPE>
__global__ void __launch_bounds__(PNL_NTHREADS)
k_h2_leaf_values(const DevProblem P, const H2Dev H, int nq, const double *__restrict__ qbary, const double *__restrict__ qw,
                 const double *__restrict__ qphi) {
    constexpr int NV = DIM+1;
    const int lf = blockIdx.x, node = H.leaf_node[lf];
    const double *bx = H.box+(size_t)node*DIM*2;
    const int *dofs = H.leaf_dofs+H.leaf_dof_off[lf];
    const int nd = H.leaf_dof_off[lf+1]-H.leaf_dof_off[lf];
    const int *cells = H.leaf_cells+H.leaf_cell_off[lf];
    const int ncl = H.leaf_cell_off[lf+1]-H.leaf_cell_off[lf];
    double *V = H.V+H.leaf_val_off[lf];
    // Chebyshev nodes of the leaf's box, once per workgroup (the cosines were 3/4 of the kernel: 5.2 -> 1.x ms at 49k DoFs)
    constexpr int MAXM = 64;
    __shared__ double s_node[DIM][MAXM];
    const bool tab = H.m <= MAXM;
    if (tab) {
        for (int t = threadIdx.x; t < DIM*H.m; t += PNL_NTHREADS) s_node[t/H.m][t % H.m] = cheb_node(bx[2*(t/H.m)], bx[2*(t/H.m)+1], H.m, t % H.m);
        __syncthreads();
    }
    for (int t = threadIdx.x; t < ncl*H.M; t += PNL_NTHREADS) {
        const int c = cells[t/H.M], alpha = t % H.M;
        int lcl[DPE];
        bool any = false;
#pragma unroll
        for (int k = 0; k < DPE; k++) {
            const int I = P.cdof[(size_t)k*P.ncp+c];
            int lo = 0, hi = nd;
            while (lo < hi) { const int mid = (lo+hi) >> 1; if (dofs[mid] < I) lo = mid+1; else hi = mid; }
            lcl[k] = (I >= 0 && lo < nd && dofs[lo] == I) ? lo : -1;
            any = any || lcl[k] >= 0;
        }
        if (!any) continue;
        double acc[DPE];
#pragma unroll
        for (int k = 0; k < DPE; k++) acc[k] = 0.;
        const double vol = P.cvol[c];
        for (int j = 0; j < nq; j++) {
            double L = 1.;
            int aa = alpha;
#pragma unroll
            for (int d = 0; d < DIM; d++) {
                double x = 0.;
#pragma unroll
                for (int v = 0; v < NV; v++) x = __builtin_fma(qbary[3*j+v], P.cellv[(size_t)(v*DIM+d)*P.ncp+c], x);
                const int l = aa % H.m;
                if (tab) {
                    // lagrange1d with the nodes from the table: the same operations in the same order
                    const double xl = s_node[d][l];
                    double v = 1.;
                    for (int k = 0; k < H.m; k++)
                        if (k != l) { const double xk = s_node[d][k]; v *= (x-xk)/(xl-xk); }
                    L *= v;
                } else L *= lagrange1d(bx[2*d], bx[2*d+1], H.m, l, x);
                aa /= H.m;
            }
            const double wl = vol*qw[j]*L;
#pragma unroll
            for (int k = 0; k < DPE; k++) acc[k] = __builtin_fma(wl, qphi[j*DPE+k], acc[k]);
        }
#pragma unroll
        for (int k = 0; k < DPE; k++)
            if (lcl[k] >= 0) atomic_add_f64(&V[(size_t)lcl[k]*H.M+alpha], acc[k]);
    }
}

// upward pass, leaves: cup[node][alpha] = sum_dofs x[dof] V[dof][alpha]
__global__ void __launch_bounds__(64)
k_h2_up_leaves(const H2Dev H, const double *__restrict__ x) {
    const int lf = blockIdx.x, node = H.leaf_node[lf];
    const int *dofs = H.leaf_dofs+H.leaf_dof_off[lf];
    const int nd = H.leaf_dof_off[lf+1]-H.leaf_dof_off[lf];
    const double *V = H.V+H.leaf_val_off[lf];
    for (int a = threadIdx.x; a < H.M; a += 64) {
        double s = 0.;
        for (int k = 0; k < nd; k++) s = __builtin_fma(x[dofs[k]], V[(size_t)k*H.M+a], s);
        H.cup[(size_t)node*H.M+a] = s;
    }
}

// y[i] += sum_j B[i][j] x[j] for a row-major M x M block, one wave: the lanes run over the COLUMNS, so a row is read as contiguous
// segments (a lane per row reads with a stride of M doubles: 64 cache lines per load), one wave reduction per row; lane i keeps row i and
// the results leave as one coalesced set of atomics per 64 rows
__device__ __forceinline__ void h2_block_matvec_add(const double *__restrict__ B, int M, const double *__restrict__ x, double *__restrict__ y) {
    const int lane = threadIdx.x & 63;
    for (int i0 = 0; i0 < M; i0 += 64) {
        double mine = 0.;
        const int rows = min(64, M-i0);
        for (int ii = 0; ii < rows; ii++) {
            const double *__restrict__ row = B+(size_t)(i0+ii)*M;
            double s = 0.;
            for (int j = lane; j < M; j += 64) s = __builtin_fma(row[j], x[j], s);
            s = wave_sum(s);
            mine = (lane == ii) ? s : mine;
        }
        if (lane < rows) atomic_add_f64(&y[i0+lane], mine);
    }
}

// upward pass, one level: cup[parent] += T_child cup[child] for the nodes of the level (list of children)
__global__ void __launch_bounds__(64)
k_h2_up_level(const H2Dev H, const int *__restrict__ nodes, int n) {
    const int c = nodes[blockIdx.x], p = H.parent[c];
    (void)n;
    h2_block_matvec_add(H.T+(size_t)c*H.M*H.M, H.M, H.cup+(size_t)c*H.M, H.cup+(size_t)p*H.M);
}

// far field: cdown[n1] += K cup[n2]
__global__ void __launch_bounds__(64)
k_h2_far(const H2Dev H) {
    const int pr = blockIdx.x, n1 = H.far[2*pr], n2 = H.far[2*pr+1];
    h2_block_matvec_add(H.K+(size_t)pr*H.M*H.M, H.M, H.cup+(size_t)n2*H.M, H.cdown+(size_t)n1*H.M);
}

// downward pass, one level: cdown[child] += T_child^T cdown[parent]
__global__ void __launch_bounds__(64)
k_h2_down_level(const H2Dev H, const int *__restrict__ nodes, int n) {
    const int c = nodes[blockIdx.x], p = H.parent[c];
    (void)n;
    const double *T = H.T+(size_t)c*H.M*H.M;
    for (int j = threadIdx.x; j < H.M; j += 64) {
        double s = 0.;
        for (int i = 0; i < H.M; i++) s = __builtin_fma(T[(size_t)i*H.M+j], H.cdown[(size_t)p*H.M+i], s);
        H.cdown[(size_t)c*H.M+j] += s;           // every child is written by one workgroup, after its parent's level
    }
}

// downward pass, leaves: y[dof] += sum_alpha V[dof][alpha] cdown[node][alpha]
__global__ void __launch_bounds__(64)
k_h2_down_leaves(const H2Dev H, double *__restrict__ y) {
    const int lf = blockIdx.x, node = H.leaf_node[lf];
    const int *dofs = H.leaf_dofs+H.leaf_dof_off[lf];
    const int nd = H.leaf_dof_off[lf+1]-H.leaf_dof_off[lf];
    const double *V = H.V+H.leaf_val_off[lf];
    for (int k = threadIdx.x; k < nd; k += 64) {
        double s = 0.;
        for (int a = 0; a < H.M; a++) s = __builtin_fma(V[(size_t)k*H.M+a], H.cdown[(size_t)node*H.M+a], s);
        y[dofs[k]] += s;                         // leaves partition the DoFs
    }
}

extern "C" {

int pnl_h2_setup(pnl_context *ctx, const pnl_h2_plan *pl) {
    if (!ctx || !pl) return PNL_ERR_INVALID;
    int rc;
    if (ctx->have_pw) {
        // order per quadrature point: no kernel block of a class, the order function evaluates s(x) (pnl_pwnear.hip)
        if (ctx->pw.type == 5) return fail(ctx, PNL_ERR_UNSUPPORTED, "H2 far field of an order given as a finite element function");
        if ((rc = pnl_pw_prepare(ctx, 0))) return rc;
    } else {
    if ((rc = pnl_assembly_prepare(ctx))) return rc;
    // finite horizon: every admissible pair must lie inside it (pnl_tree_build_horizon drops the pairs beyond the horizon and keeps the
    // ones it may cut in the near field, clusterMethodCy.pyx:4069-4090); the interpolants are those of the kernel itself
    if (!std::isinf(ctx->C().kern[0].horizon2)) {
        if (ctx->have_xform) return fail(ctx, PNL_ERR_UNSUPPORTED, "H2 far field of a finite horizon: l2 ball only");
        if (!pl->box || (pl->nfar > 0 && !pl->far)) return PNL_ERR_INVALID;
        const double h2 = ctx->C().kern[0].horizon2;
        for (int p = 0; p < pl->nfar; p++) {
            const double *a = pl->box+(size_t)pl->far[2*p]*ctx->dim*2, *b = pl->box+(size_t)pl->far[2*p+1]*ctx->dim*2;
            // maxDistBoxes as the reference writes it (interactionDomains.pyx:325-337): what its admissibility test compares with the
            // horizon; interpolation nodes that do lie beyond the horizon get the kernel value 0 there and here (kern_eval)
            double d2 = 0.;
            for (int d = 0; d < ctx->dim; d++) {
                const bool first = a[2*d] > b[2*d];
                const double e = std::max((first ? a[2*d+1] : b[2*d+1])-(first ? b[2*d] : a[2*d]), 0.);
                d2 += e*e;
            }
            if (d2 > h2*(1.+1e-12))
                return fail(ctx, PNL_ERR_INVALID, "H2 far field: the clusters of admissible pair %d reach beyond the horizon", p);
        }
    }
    }
    // (the admissible pairs are ORDERED -- (n1, n2) and (n2, n1) are two entries, each with the class of its orientation -- so a
    // non-symmetric order table needs nothing beyond its far_class)
    if (ctx->nlab > 0 && pl->nfar > 0 && !pl->far_class)
        return fail(ctx, PNL_ERR_UNSUPPORTED, "H2 far field of a variable order: a kernel class per admissible pair is needed");
    if (pl->far_class)
        for (int i = 0; i < pl->nfar; i++)
            if (pl->far_class[i] < 0 || pl->far_class[i] >= (int)ctx->cls.size()) return fail(ctx, PNL_ERR_INVALID, "far pair %d: bad kernel class", i);
    const int dim = ctx->dim, m = pl->m;
    if (pl->nnodes <= 0 || pl->nleaves <= 0 || pl->nfar < 0 || m < 1 || m > 16 || pl->nq <= 0) return fail(ctx, PNL_ERR_INVALID, "bad H2 plan sizes");
    int M = 1;
    for (int d = 0; d < dim; d++) M *= m;
    int nroot = 0;
    for (int n = 0; n < pl->nnodes; n++) {
        if (pl->parent[n] < -1 || pl->parent[n] >= pl->nnodes || pl->level[n] < 0 || pl->level[n] >= pl->nlevels)
            return fail(ctx, PNL_ERR_INVALID, "node %d: bad parent / level", n);
        if (pl->parent[n] < 0) nroot++;
        else if (pl->level[pl->parent[n]] != pl->level[n]-1) return fail(ctx, PNL_ERR_INVALID, "node %d: level is not its parent's + 1", n);
    }
    if (nroot != 1) return fail(ctx, PNL_ERR_INVALID, "the tree needs exactly one root");
    for (int i = 0; i < 2*pl->nfar; i++)
        if (pl->far[i] < 0 || pl->far[i] >= pl->nnodes) return fail(ctx, PNL_ERR_INVALID, "far pair out of range");
    std::vector<long long> voff(pl->nleaves);
    long long vtot = 0;
    std::vector<char> covered(ctx->N, 0);
    for (int l = 0; l < pl->nleaves; l++) {
        if (pl->leaf_node[l] < 0 || pl->leaf_node[l] >= pl->nnodes) return fail(ctx, PNL_ERR_INVALID, "leaf %d: bad node", l);
        voff[l] = vtot;
        vtot += (long long)(pl->leaf_dof_off[l+1]-pl->leaf_dof_off[l])*M;
        for (int t = pl->leaf_dof_off[l]; t < pl->leaf_dof_off[l+1]; t++) {
            const int I = pl->leaf_dofs[t];
            if (I < 0 || I >= ctx->N || covered[I] || (t > pl->leaf_dof_off[l] && pl->leaf_dofs[t-1] >= I))
                return fail(ctx, PNL_ERR_INVALID, "leaf %d: DoFs must be sorted and the leaves must partition the DoFs", l);
            covered[I] = 1;
        }
        for (int t = pl->leaf_cell_off[l]; t < pl->leaf_cell_off[l+1]; t++)
            if (pl->leaf_cells[t] < 0 || pl->leaf_cells[t] >= ctx->nc) return fail(ctx, PNL_ERR_INVALID, "leaf %d: bad cell", l);
    }
    if (!pl->partial_leaves)
        for (int I = 0; I < ctx->N; I++)
            if (!covered[I]) return fail(ctx, PNL_ERR_INVALID, "DoF %d belongs to no leaf (set partial_leaves for a rank-local plan)", I);
    DevBuf *B = ctx->b_h2;
    H2Dev &H = ctx->h2;
    std::memset(&H, 0, sizeof(H));
    H.dim = dim; H.m = m; H.M = M; H.nnodes = pl->nnodes; H.nleaves = pl->nleaves; H.nfar = pl->nfar;
    if ((rc = upload(ctx, B[0], pl->box, (size_t)pl->nnodes*dim*2))) return rc;
    if ((rc = upload(ctx, B[1], pl->parent, (size_t)pl->nnodes))) return rc;
    if ((rc = upload(ctx, B[2], pl->leaf_node, (size_t)pl->nleaves))) return rc;
    if ((rc = upload(ctx, B[3], pl->leaf_dof_off, (size_t)pl->nleaves+1))) return rc;
    if ((rc = upload(ctx, B[4], pl->leaf_dofs, (size_t)pl->leaf_dof_off[pl->nleaves]))) return rc;
    if ((rc = upload(ctx, B[5], pl->leaf_cell_off, (size_t)pl->nleaves+1))) return rc;
    if ((rc = upload(ctx, B[6], pl->leaf_cells, (size_t)pl->leaf_cell_off[pl->nleaves]))) return rc;
    if ((rc = upload(ctx, B[7], voff.data(), voff.size()))) return rc;
    ctx->h2_vtot = vtot;
    if ((rc = upload(ctx, B[8], pl->far, (size_t)2*pl->nfar))) return rc;
    if ((rc = upload(ctx, B[9], pl->transfer, (size_t)pl->nnodes*M*M))) return rc;
    if ((rc = ensure(ctx, B[10], sizeof(double)*(size_t)std::max<long long>(vtot, 1)))) return rc;
    if ((rc = ensure(ctx, B[11], sizeof(double)*(size_t)std::max(pl->nfar, 1)*M*M))) return rc;
    if ((rc = ensure(ctx, B[12], sizeof(double)*(size_t)pl->nnodes*M))) return rc;
    if ((rc = ensure(ctx, B[13], sizeof(double)*(size_t)pl->nnodes*M))) return rc;
    if ((rc = upload(ctx, B[14], pl->qbary, (size_t)3*pl->nq))) return rc;
    if ((rc = upload(ctx, B[15], pl->qw, (size_t)pl->nq))) return rc;
    if ((rc = upload(ctx, B[16], pl->qphi, (size_t)pl->nq*ctx->dpe))) return rc;
    H.box = (const double*)B[0].p; H.parent = (const int*)B[1].p; H.leaf_node = (const int*)B[2].p;
    H.leaf_dof_off = (const int*)B[3].p; H.leaf_dofs = (const int*)B[4].p; H.leaf_cell_off = (const int*)B[5].p;
    H.leaf_cells = (const int*)B[6].p; H.leaf_val_off = (const long long*)B[7].p; H.far = (const int*)B[8].p;
    H.T = (const double*)B[9].p; H.V = (double*)B[10].p; H.K = (double*)B[11].p; H.cup = (double*)B[12].p; H.cdown = (double*)B[13].p;
    // nodes per level (children lists), concatenated on the device
    ctx->h2_levels.assign(pl->nlevels, std::vector<int>());
    for (int n = 0; n < pl->nnodes; n++)
        if (pl->parent[n] >= 0) ctx->h2_levels[pl->level[n]].push_back(n);
    std::vector<int> cat;
    ctx->h2_level_off.assign(pl->nlevels+1, 0);
    for (int l = 0; l < pl->nlevels; l++) {
        ctx->h2_level_off[l] = cat.size();
        cat.insert(cat.end(), ctx->h2_levels[l].begin(), ctx->h2_levels[l].end());
    }
    ctx->h2_level_off[pl->nlevels] = cat.size();
    if ((rc = upload(ctx, B[17], cat.data(), cat.size()))) return rc;
    if ((rc = pnl_h2_block_plan(ctx, pl))) return rc;
    HIPCHK(ctx, hipMemsetAsync(H.V, 0, sizeof(double)*(size_t)std::max<long long>(vtot, 1), ctx->stream));
    const double *qb = (const double*)B[14].p, *qw = (const double*)B[15].p, *qp = (const double*)B[16].p;
    if ((rc = with_shape(ctx, [&](auto D, auto E) {
            hipLaunchKernelGGL((k_h2_leaf_values<decltype(D)::value, decltype(E)::value>), dim3(pl->nleaves), dim3(PNL_NTHREADS), 0, ctx->stream,
                               ctx->P, H, pl->nq, qb, qw, qp);
            return PNL_OK;
        }))) return rc;
    if (pl->nfar > 0) {
        const DevKernel *kcls = nullptr;
        const int *fcls = nullptr;
        if (pl->far_class) {
            std::vector<DevKernel> kc;
            for (auto *c : ctx->cls) kc.push_back(to_dev(c->kern[0], dim));
            if ((rc = upload(ctx, B[18], kc.data(), kc.size()))) return rc;
            if ((rc = upload(ctx, B[19], pl->far_class, (size_t)pl->nfar))) return rc;
            kcls = (const DevKernel*)B[18].p; fcls = (const int*)B[19].p;
        }
        if (ctx->have_pw) {
            // order per quadrature point: the kernel with the order at the nodes of the row cluster (pnl_pwnear.hip)
            if ((rc = pnl_pw_h2_interp(ctx))) return rc;
        } else
        if (dim == 2) hipLaunchKernelGGL((k_h2_kernel_interp<2>), dim3(pl->nfar), dim3(PNL_NTHREADS), 0, ctx->stream, ctx->P, H, kcls, fcls);
        else hipLaunchKernelGGL((k_h2_kernel_interp<1>), dim3(pl->nfar), dim3(PNL_NTHREADS), 0, ctx->stream, ctx->P, H, kcls, fcls);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->have_h2 = true;
    return PNL_OK;
}

// the three phases of the H2 matvec on the coefficient arrays H.cup / H.cdown (the context's own, or the caller's)
static int h2_upward(pnl_context *ctx, const H2Dev &H, const double *x) {
    const int nlev = (int)ctx->h2_levels.size();
    const int *lev = (const int*)ctx->b_h2[17].p;
    HIPCHK(ctx, hipMemsetAsync(H.cup, 0, sizeof(double)*(size_t)H.nnodes*H.M, ctx->stream));
    hipLaunchKernelGGL(k_h2_up_leaves, dim3(H.nleaves), dim3(64), 0, ctx->stream, H, x);
    for (int l = nlev-1; l >= 1; l--) {
        const int n = (int)ctx->h2_levels[l].size();
        if (n) hipLaunchKernelGGL(k_h2_up_level, dim3(n), dim3(64), 0, ctx->stream, H, lev+ctx->h2_level_off[l], n);
    }
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}
static int h2_interact(pnl_context *ctx, const H2Dev &H) {
    HIPCHK(ctx, hipMemsetAsync(H.cdown, 0, sizeof(double)*(size_t)H.nnodes*H.M, ctx->stream));
    if (H.nfar) hipLaunchKernelGGL(k_h2_far, dim3(H.nfar), dim3(64), 0, ctx->stream, H);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}
static int h2_downward(pnl_context *ctx, const H2Dev &H, double *y) {
    const int nlev = (int)ctx->h2_levels.size();
    const int *lev = (const int*)ctx->b_h2[17].p;
    for (int l = 1; l < nlev; l++) {
        const int n = (int)ctx->h2_levels[l].size();
        if (n) hipLaunchKernelGGL(k_h2_down_level, dim3(n), dim3(64), 0, ctx->stream, H, lev+ctx->h2_level_off[l], n);
    }
    hipLaunchKernelGGL(k_h2_down_leaves, dim3(H.nleaves), dim3(64), 0, ctx->stream, H, y);
    HIPCHK(ctx, hipGetLastError());
    return PNL_OK;
}

int pnl_h2_matvec(pnl_context *ctx, const double *x, double *y) {
    if (!ctx || !x || !y) return PNL_ERR_INVALID;
    if (!ctx->have_h2) return fail(ctx, PNL_ERR_STATE, "pnl_h2_setup first");
    int rc;
    if ((rc = h2_upward(ctx, ctx->h2, x)) || (rc = h2_interact(ctx, ctx->h2))) return rc;
    return h2_downward(ctx, ctx->h2, y);
}

// kernel interpolants K[nfar][M][M] (which = 0) and leaf values V (which = 1: the blocks V_leaf[ndofs][M] of the plan's leaves, one
// after the other) between the device and the host: the H2 operator file (clusterMethodCy.pyx:2449-2550) stores them
static int h2_copy(pnl_context *ctx, int which, double *host, bool to_host) {
    if (!ctx || !host) return PNL_ERR_INVALID;
    if (!ctx->have_h2) return fail(ctx, PNL_ERR_STATE, "pnl_h2_setup first");
    if (which != 0 && which != 1) return fail(ctx, PNL_ERR_INVALID, "pnl_h2_get / _set: which = 0 (interpolants) or 1 (leaf values)");
    const H2Dev &H = ctx->h2;
    const size_t n = which == 0 ? (size_t)H.nfar*H.M*H.M : (size_t)ctx->h2_vtot;
    double *dev = which == 0 ? H.K : H.V;
    if (n) HIPCHK(ctx, hipMemcpyAsync(to_host ? (void*)host : (void*)dev, to_host ? (const void*)dev : (const void*)host, n*sizeof(double),
                                      to_host ? hipMemcpyDeviceToHost : hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return PNL_OK;
}
int pnl_h2_get(pnl_context *ctx, int which, double *dst_host) { return h2_copy(ctx, which, dst_host, true); }
int pnl_h2_set(pnl_context *ctx, int which, const double *src_host) { return h2_copy(ctx, which, const_cast<double*>(src_host), false); }

int pnl_h2_sizes(pnl_context *ctx, int32_t *out2) {
    if (!ctx || !out2) return PNL_ERR_INVALID;
    if (!ctx->have_h2) return fail(ctx, PNL_ERR_STATE, "pnl_h2_setup first");
    out2[0] = ctx->h2.nnodes; out2[1] = ctx->h2.M;
    return PNL_OK;
}

int pnl_h2_upward(pnl_context *ctx, const double *x, double *cup) {
    if (!ctx || !x || !cup) return PNL_ERR_INVALID;
    if (!ctx->have_h2) return fail(ctx, PNL_ERR_STATE, "pnl_h2_setup first");
    H2Dev H = ctx->h2;
    H.cup = cup;
    return h2_upward(ctx, H, x);
}

int pnl_h2_interact(pnl_context *ctx, const double *cup, double *cdown) {
    if (!ctx || !cup || !cdown) return PNL_ERR_INVALID;
    if (!ctx->have_h2) return fail(ctx, PNL_ERR_STATE, "pnl_h2_setup first");
    H2Dev H = ctx->h2;
    H.cup = const_cast<double*>(cup); H.cdown = cdown;
    return h2_interact(ctx, H);
}

int pnl_h2_downward(pnl_context *ctx, double *cdown, double *y) {
    if (!ctx || !cdown || !y) return PNL_ERR_INVALID;
    if (!ctx->have_h2) return fail(ctx, PNL_ERR_STATE, "pnl_h2_setup first");
    H2Dev H = ctx->h2;
    H.cdown = cdown;
    return h2_downward(ctx, H, y);
}
}  // extern "C"
