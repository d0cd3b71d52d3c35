// Internal, host only: runtime value -> template argument.  f receives std::integral_constants and returns the launcher's code.
// Needs pnl_context.h only and names no kernel, so that a unit without the kernels of pnl_kernels.h (pnl_h2.hip) can include it;
// pnl_launch.h, whose templates do name those kernels, brings it.
#pragma once
#include <type_traits>

// number of common vertices - 1 of a touching pair -> SLOT of its rule (the last slot of the dimension: identical cells)
template <int DIM, class F>
static int with_slot(int s, F &&f) {
    if (s == 0) return f(std::integral_constant<int, 0>{});
    if (s == 1) return f(std::integral_constant<int, 1>{});
    return f(std::integral_constant<int, (DIM == 2 ? 2 : 1)>{});
}
// quarter-integer exponent (DevKernel::fast) -> KT 1, general exponent -> KT 0
template <class F>
static int with_kt(bool fast, F &&f) {
    return fast ? f(std::integral_constant<int, 1>{}) : f(std::integral_constant<int, 0>{});
}
// the same where the intervals are instantiated with KT = 0 only (masked pairs, finite horizon): with_kt for DIM == 2
template <int DIM, class F>
static int with_kt_2d(bool fast, F &&f) {
    if constexpr (DIM == 2) return with_kt(fast, f);
    else return f(std::integral_constant<int, 0>{});
}
// (dim, dofs per element) of the context -> DIM, DPE: triangles P1, P2, P0 and intervals P1, P2, P0, P3, the shapes finalize() takes
// (P0 and P3 on intervals: the reference's fixtures --elementP0 / --elementP3; FL1 is generic in the DoFs per element)
template <class F>
static int with_shape(pnl_context *ctx, F &&f) {
    using std::integral_constant;
    const int dim = ctx->dim, dpe = ctx->dpe;
    if (dim == 2 && dpe == 3) return f(integral_constant<int, 2>{}, integral_constant<int, 3>{});
    if (dim == 2 && dpe == 6) return f(integral_constant<int, 2>{}, integral_constant<int, 6>{});
    if (dim == 2 && dpe == 1) return f(integral_constant<int, 2>{}, integral_constant<int, 1>{});
    if (dim == 1 && dpe == 2) return f(integral_constant<int, 1>{}, integral_constant<int, 2>{});
    if (dim == 1 && dpe == 3) return f(integral_constant<int, 1>{}, integral_constant<int, 3>{});
    if (dim == 1 && dpe == 1) return f(integral_constant<int, 1>{}, integral_constant<int, 1>{});
    if (dim == 1 && dpe == 4) return f(integral_constant<int, 1>{}, integral_constant<int, 4>{});
    return fail(ctx, PNL_ERR_UNSUPPORTED, "unsupported (dim=%d, dofs_per_element=%d)", dim, dpe);
}
// cells per tile of a shape: TILE_P2 exactly where an element has more DoFs than vertices (P2, P3), TILE_P1 otherwise
template <int DIM, int DPE>
constexpr int tile_cells = DPE > DIM+1 ? TILE_P2 : TILE_P1;
