// water_column.hip -- the kernels of the water column (water_column.h): the layer builder's weight kernel and both instantiations of
// the column query, and the draught kernels of the hull family (hull_draught.h), compiled without floating-point contraction.  As in surface_tiled.hip the pragma stands after mw_math.h, which sets
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

// The grid mapping of k_hull_triangles, k_hull_reduce and k_bodies_integrate over the functions those call.  None reads the mesh, so
// one form serves the one footprint and the tiling.
__global__ __launch_bounds__(256) void k_draught_triangles(HullArgs a) {
    const int l = threadIdx.x;
    const int64_t total = a.nbodies * a.nchunks;
    for (int64_t blk = blockIdx.x; blk < total; blk += gridDim.x) {
        const int64_t b = blk / a.nchunks;
        const int c = (int)(blk - b * a.nchunks);
        const float* vs = reinterpret_cast<const float*>(a.vslab + 2 * b * a.nverts);
        float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float res = 0.f;
        const int t = c * MW_HULL_CHUNK + l;
        if (t < a.ntris) {
            float body[16];
            hull_load_body(a.bodies + 4 * b, body);
            const int idx[3] = {a.tris[3 * (size_t)t], a.tris[3 * (size_t)t + 1], a.tris[3 * (size_t)t + 2]};
            if (!hull_triangle(idx, a.nverts, vs, body, a.cf, acc)) res = NAN;
        }
        if (t < a.nverts) res = hull_max(res, vs[8 * (size_t)t + 7]);
        hull_chunk_partial(acc, res, a.part + 2 * blk);
    }
}

__global__ __launch_bounds__(256) void k_draught_reduce(HullArgs a) {
    const int l = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t b = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; b < a.nbodies; b += nwaves) {  // wave-uniform
        float acc[7], res;
        hull_body_sum(a.part, b * a.nchunks, a.nchunks, l, acc, res);
        if (l == 0) {
            float o[8];
            hull_row(acc, res, o);
            hull_store_row(a.out + 2 * b, o);
        }
    }
}

__global__ __launch_bounds__(256) void k_draught_integrate(BodiesArgs a) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.h.nbodies) return;
    float body[16], mass[8], row[8];
    hull_load_body(a.bodies + 4 * b, body);
    hull_load_row(a.mass + 2 * b, mass);
    hull_load_row(a.rows + 2 * b, row);
    if (!body_mass_valid(mass)) {
        for (int k = 0; k < 8; k++) row[k] = NAN;
    } else if (body_integrate(body, row, mass, a.g, a.dt)) {
        for (int k = 0; k < 4; k++) a.bodies[4 * b + k] = make_float4(body[4 * k], body[4 * k + 1], body[4 * k + 2], body[4 * k + 3]);
    }
    if (a.last && a.out) hull_store_row(a.out + 2 * b, row);
}

hipError_t draught_forces_launch(hipStream_t s, dim3 gv, dim3 gt, dim3 gr, const HullArgs& a, const ColTable& tb) {
    if (a.m.period != 0.f) {
        const DraughtArgsT<SqTiled> v{SqTiled{a.m}, tb, a.cf.drag, a.vscale, a.iters, a.hull, a.bodies, a.nverts, a.nbodies, a.vslab};
        k_draught_vertices<<<gv, dim3(256), 0, s>>>(v);
    } else {
        const DraughtArgsT<SqMesh> v{a.m, tb, a.cf.drag, a.vscale, a.iters, a.hull, a.bodies, a.nverts, a.nbodies, a.vslab};
        k_draught_vertices<<<gv, dim3(256), 0, s>>>(v);
    }
    k_draught_triangles<<<gt, dim3(MW_HULL_CHUNK), 0, s>>>(a);
    k_draught_reduce<<<gr, dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t draught_integrate_launch(hipStream_t s, dim3 gi, const BodiesArgs& a) {
    k_draught_integrate<<<gi, dim3(256), 0, s>>>(a);
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
