// water_column.hip -- the kernels of the water column (water_column.h): the layer builder's weight kernel and both instantiations of
// the column query, and the one kernel draught adds to the hull family (hull_draught.h): k_draught_vertices, both instantiations.  It
// stands here because it needs water_column.h; the kernels that read its slab do not (they read no mesh at all, hull_forces.h) and are
// surface_tiled.hip's.  Compiled without floating-point contraction.  As in surface_tiled.hip the pragma stands after mw_math.h, which sets
// its own inside its strict helpers, and before the headers whose MW_HD functions the kernels run: the column is the strict float32 the
// g++ build of the same functions computes (tests/column_shim.cpp), on a periodic handle and on the one footprint alike.
#include <hip/hip_runtime.h>

#include "mw_math.h"
#pragma clang fp contract(off)
#define MW_VEL_NO_KERNELS  // velocity_weight alone: the velocity kernels are mistral_water.hip's
#define MW_COL_KERNELS
#include "water_column.h"
#include "hull_draught.h"

namespace mw {

// ---- draught (hull_draught.h): the hull family on the column ----
// One lane per instance vertex (n = nbodies * nverts < 2^31), as k_hull_vertices: the body's 64 B, the layer scan of col_world_point
// (the table is a kernel argument, read with the loop's wave-uniform index), two 16-byte stores.  No LDS, no atomics.
template <typename Mesh>
__global__ __launch_bounds__(256) void k_draught_vertices(DraughtArgsT<Mesh> a) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.nbodies * a.nverts) return;
    const unsigned b = (unsigned)k / (unsigned)a.nverts;  // k < 2^31
    const int v = (int)((unsigned)k - b * (unsigned)a.nverts);
    float body[16], h[3], s[8];
    hull_load_body(a.bodies + 4 * (size_t)b, body);
    for (int c = 0; c < 3; c++) h[c] = a.hull[3 * (size_t)v + c];
    hull_vertex_draught(a.m, a.tb, a.drag, a.vscale, a.iters, body, h, s);
    hull_store_row(a.vslab + 2 * k, s);
}

// The vertex phase alone: the kernels after the slab are surface_tiled.hip's strict ones (strict_hull_rows, strict_bodies_integrate).
hipError_t draught_vertices_launch(hipStream_t s, dim3 gv, const HullArgs& a, const ColTable& tb) {
    if (a.m.period != 0.f) {
        const DraughtArgsT<SqTiled> v{SqTiled{a.m}, tb, a.cf.drag, a.vscale, a.iters, a.hull, a.bodies, a.nverts, a.nbodies, a.vslab};
        k_draught_vertices<<<gv, dim3(256), 0, s>>>(v);
    } else {
        const DraughtArgsT<SqMesh> v{a.m, tb, a.cf.drag, a.vscale, a.iters, a.hull, a.bodies, a.nverts, a.nbodies, a.vslab};
        k_draught_vertices<<<gv, dim3(256), 0, s>>>(v);
    }
    return hipGetLastError();
}

hipError_t column_weight_launch(hipStream_t s, int N, float length, float gravity, float depth, const cf* h0, const cf* h0c, cf* ph0, cf* ph0c,
                                cf* vh0, cf* vh0c) {
    const unsigned nb = (unsigned)(((size_t)N * N + 255) / 256);
    k_column_weight<<<dim3(nb), dim3(256), 0, s>>>(N, length, gravity, depth, h0, h0c, ph0, ph0c, vh0, vh0c);
    return hipGetLastError();
}

hipError_t column_query_launch(hipStream_t s, const SqMesh& m, const ColTable& tb, int mode, int iters, const float4* xyz, int64_t n, float4* out) {
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    if (m.period != 0.f) k_query_column<<<grid, block, 0, s>>>(SqTiled{m}, tb, mode, iters, xyz, n, out);
    else k_query_column<<<grid, block, 0, s>>>(m, tb, mode, iters, xyz, n, out);
    return hipGetLastError();
}

}  // namespace mw
