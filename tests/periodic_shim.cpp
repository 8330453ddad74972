// tests/periodic_shim.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The MW_HD functions of the surface services (mistral-water_amd/csrc/surface_query.h, hull_forces.h, rigid_bodies.h) compiled with g++
// over a mesh read as its infinite tiling (SqTiled, period != 0) or as the one footprint (SqMesh, period == 0): the surface and velocity
// queries, the hull vertex step, the rows summed in the kernels' own order, and the substep chain of the bodies in both plans' order
// (the order is tests/hull_order.h's hand restatement, shared with draught_shim.cpp; the vertex step is this file's).
// The tiled kernels are built without floating-point contraction (csrc/surface_tiled.hip), so what this file computes for period != 0 is
// what the device computes, bit for bit (tests/test_periodic_gpu.py).  Never part of libmistral_water.so and not a fallback.
//
// build: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared (tests/periodic_ref.py::build_shim)
#include <cstdint>

#include "hull_order.h"

using namespace mw;

namespace {
SqMesh mesh_of(int R, float uw, float period, const float* vert, const float* norm, const float* white, int wstride) {
    SqMesh m{vert, norm, white, R, wstride, uw};
    m.period = period;
    return m;
}
bool bad(int R, float uw, int iters) { return R < 2 || !(uw > 0.f) || iters < 0 || iters > MW_SQ_MAX_ITERS; }
int its(int iters) { return iters == 0 ? MW_SQ_DEFAULT_ITERS : iters; }

// the vertex step of one body over the mesh, as hull_order takes it
template <typename Mesh>
auto vertices_of(const Mesh& m, const float* vel, float vscale, int iters, const float* hull, int nverts) {
    return [=](const float body[16], float* slab) {
        for (int v = 0; v < nverts; v++) hull_vertex(m, vel, vscale, iters, body, hull + 3 * v, slab + 8 * (size_t)v);
    };
}

// A hull export's arguments as hull_order takes them: run(call, vertices) gets the vertex step on the mesh type the period selects.
// 1: bad arguments
template <typename Run>
int hull_call(int R, float uw, float period, const float* vert, const float* vel, int iters, const float* hull, int nverts, const int* tris,
              int ntris, const float* coeffs, float dt, int substeps, Run run) {
    if (bad(R, uw, iters) || substeps < 1) return 1;
    const SqMesh m = mesh_of(R, uw, period, vert, vert, vert, 3);  // normals / whitecap are not read
    HullCoeffs cf;
    float g, vscale;
    hull_coeffs(coeffs, &cf, &g, &vscale);
    const float* u = cf.drag ? vel : nullptr;
    const hull_order::Call c{tris, nverts, ntris, cf, g, dt / (float)substeps, substeps};
    if (period != 0.f) run(c, vertices_of(SqTiled{m}, u, vscale, its(iters), hull, nverts));
    else run(c, vertices_of(m, u, vscale, its(iters), hull, nverts));
    return 0;
}
}  // namespace

// P = (float)N * unit_width and the rest coordinate of grid line g of the tiling
extern "C" float ps_period(int N, float unit_width) { return (float)N * unit_width; }
extern "C" float ps_rest(int N, float unit_width, int g) { return sq_tiled_rest(N, unit_width, (float)N * unit_width, g); }

// the launch arithmetic of a hull call: its chunks, the dynamic LDS of the one-launch plan and that plan's limit
extern "C" int ps_hull_chunks(int nverts, int ntris) { return hull_chunks(nverts, ntris); }
extern "C" int64_t ps_bodies_step_lds(int nverts, int nchunks) { return (int64_t)bodies_step_lds(nverts, nchunks); }
extern "C" int64_t ps_bodies_lds_max() { return MW_BODIES_LDS_MAX; }

// sq_query_point over n points; period == 0: the one footprint
extern "C" int ps_query(int R, float unit_width, float period, const float* vert, const float* norm, const float* white, int wstride, int mode,
                        const float* xz, int64_t n, int iters, float* out) {
    if (bad(R, unit_width, iters)) return 1;
    const SqMesh m = mesh_of(R, unit_width, period, vert, norm, white, wstride);
    for (int64_t k = 0; k < n; k++) {
        if (period != 0.f) sq_query_point(SqTiled{m}, mode, xz[2 * k], xz[2 * k + 1], its(iters), out + 8 * k);
        else sq_query_point(m, mode, xz[2 * k], xz[2 * k + 1], its(iters), out + 8 * k);
    }
    return 0;
}

// sq_velocity_point over n points
extern "C" int ps_velocity(int R, float unit_width, float period, const float* vert, const float* vel, int mode, const float* xz, int64_t n,
                           int iters, float* out) {
    if (bad(R, unit_width, iters)) return 1;
    const SqMesh m = mesh_of(R, unit_width, period, vert, vert, vert, 3);  // normals / whitecap are not read
    for (int64_t k = 0; k < n; k++) {
        if (period != 0.f) sq_velocity_point(SqTiled{m}, vel, mode, xz[2 * k], xz[2 * k + 1], its(iters), out + 4 * k);
        else sq_velocity_point(m, vel, mode, xz[2 * k], xz[2 * k + 1], its(iters), out + 4 * k);
    }
    return 0;
}

// coeffs = (density, gravity, linear_drag, quadratic_drag, velocity_scale), as mw_ocean_hull_forces takes them.
// slab [nbodies][nverts][8] (hull_vertex) and rows [nbodies][8] in the kernels' summation order; vel may be NULL (drag off)
extern "C" int ps_hull_forces(int R, float unit_width, float period, const float* vert, const float* vel, int iters, const float* hull, int nverts,
                              const int* tris, int ntris, const float* bodies, int nbodies, const float* coeffs, float* slab, float* rows) {
    return hull_call(R, unit_width, period, vert, vel, iters, hull, nverts, tris, ntris, coeffs, 0.f, 1, [&](const hull_order::Call& c, auto vertices) {
        for (int b = 0; b < nbodies; b++) hull_order::forces(c, vertices, bodies + 16 * b, slab + 8 * (size_t)b * nverts, rows + 8 * b);
    });
}

// mw_ocean_step_bodies: bodies [nbodies][16] in place, out [nbodies][8] or NULL; plan 0 per substep, 1 one launch
extern "C" int ps_step_bodies(int R, float unit_width, float period, const float* vert, const float* vel, int iters, const float* hull, int nverts,
                              const int* tris, int ntris, float* bodies, const float* mass, int nbodies, const float* coeffs, float dt,
                              int substeps, int plan, float* out) {
    return hull_call(R, unit_width, period, vert, vel, iters, hull, nverts, tris, ntris, coeffs, dt, substeps,
                     [&](const hull_order::Call& c, auto vertices) { hull_order::step_bodies(c, vertices, plan, bodies, mass, nbodies, out); });
}
