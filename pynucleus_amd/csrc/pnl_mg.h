// The multigrid object behind pnl_mg_* (include/pnl_hip.h), shared by pnl_solver.hip (single-vector cycle, pnl_mg_solve, pnl_mg_cg,
// pnl_theta_step) and pnl_mg_block.hip (the cycle and the CG for a block of right-hand sides).
#pragma once
#include "pnl_context.h"

struct pnl_mg {
    pnl_context *ctx = nullptr;
    int nlevels = 0;
    std::vector<pnl_mg_level_desc> lv;
    const double *coarse_inv = nullptr;
    double omega = 2./3.;
    int pre = 1, post = 1;
    // per level: invD (omega / diag), rhs, sol, temp
    std::vector<DevBuf> invD, rhs, sol, temp;
    DevBuf r, p, Ap, z, scal, work, h2tmp;
    double last_conv = 0.;          // preconditioned residual norm sqrt(r.Br) at the end of the last pnl_mg_cg
    // block path (pnl_mg_block.hip), allocated on the first block call and not in pnl_mg_create: per level [16][ld_l] blocks for
    // rhs, sol (levels below the finest) and temp (levels above the coarsest), ld_l = n_l rounded up to an even number; the work of
    // pnl_mg_cg_block: R, P, AP, Z [16][ld_top] and the state [16][PNL_CGB_STATE]
    std::vector<DevBuf> brhs, bsol, btemp;
    DevBuf bcg;
};
