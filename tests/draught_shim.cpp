// tests/draught_shim.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The MW_HD functions of the hull family with draught on (mistral-water_amd/csrc/hull_draught.h over water_column.h, hull_forces.h and
// rigid_bodies.h) compiled with g++ over given layer arrays, read as the one footprint (period == 0) or as their tiling (period != 0):
// the vertex step on the column, then the rows summed in the kernels' own order and the substep chain -- tests/hull_order.h's hand
// restatement, the oracle for that order, shared with periodic_shim.cpp.  With draught on every kernel of the hull family is built
// without floating-point contraction (csrc/water_column.hip the vertex kernel, csrc/surface_tiled.hip the rest), so what this file
// computes is what the device computes on the same layer arrays, bit for bit (tests/test_draught_gpu.py).  Never part of
// libmistral_water.so and not a fallback.
//
// build: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared (tests/draught_ref.py::build_shim)
#include <cstdint>

#include "../mistral-water_amd/csrc/hull_draught.h"
#include "hull_order.h"

using namespace mw;

namespace {
// the vertex step of one body on the column, as hull_order takes it
template <typename Mesh>
auto vertices_of(const Mesh& m, const ColTable& tb, int drag, float vscale, int iters, const float* hull, int nverts) {
    return [=](const float body[16], float* slab) {
        for (int v = 0; v < nverts; v++) hull_vertex_draught(m, tb, drag, vscale, iters, body, hull + 3 * v, slab + 8 * (size_t)v);
    };
}

// The arguments every export takes, as hull_order takes them: run(call, vertices) gets the vertex step on the mesh type the period
// selects.  -1: bad arguments
template <typename Run>
int hull_call(int R, float uw, float period, int L, const float* depths, const float* pos, const float* vel, int iters, const float* hull, int nverts,
              const int* tris, int ntris, const float* coeffs, float dt, int substeps, Run run) {
    if (R < 2 || !(uw > 0.f) || L < 2 || L > MW_COL_MAX_LAYERS || iters < 0 || iters > MW_SQ_MAX_ITERS || substeps < 1) return -1;
    SqMesh m{nullptr, nullptr, nullptr, R, 1, uw};
    m.period = period;
    ColTable tb{};
    tb.L = L;
    for (int l = 0; l < L; l++) {
        tb.depth[l] = depths[l];
        tb.pos[l] = pos + (size_t)l * R * R * 3;
        tb.vel[l] = vel + (size_t)l * R * R * 3;
    }
    m.vert = tb.pos[0];
    const int it = iters == 0 ? MW_SQ_DEFAULT_ITERS : iters;
    HullCoeffs cf;
    float g, vscale;
    hull_coeffs(coeffs, &cf, &g, &vscale);
    const hull_order::Call c{tris, nverts, ntris, cf, g, dt / (float)substeps, substeps};
    if (period != 0.f) run(c, vertices_of(SqTiled{m}, tb, cf.drag, vscale, it, hull, nverts));
    else run(c, vertices_of(m, tb, cf.drag, vscale, it, hull, nverts));
    return 0;
}
}  // namespace

extern "C" {

// pos, vel: [L][R*R][3] contiguous (pos[0] the surface mesh, vel[0] the surface velocity); period == 0: the one footprint.
// coeffs = (density, gravity, linear_drag, quadratic_drag, velocity_scale).  slab [nbodies][nverts][8], rows [nbodies][8].  -1: bad arguments
int ds_hull_forces(int R, float uw, float period, int L, const float* depths, const float* pos, const float* vel, int iters, const float* hull,
                   int nverts, const int* tris, int ntris, const float* bodies, int nbodies, const float* coeffs, float* slab, float* rows) {
    return hull_call(R, uw, period, L, depths, pos, vel, iters, hull, nverts, tris, ntris, coeffs, 0.f, 1, [&](const hull_order::Call& c, auto vertices) {
        for (int b = 0; b < nbodies; b++) hull_order::forces(c, vertices, bodies + 16 * b, slab + 8 * (size_t)b * nverts, rows + 8 * b);
    });
}

// mw_ocean_step_bodies with draught on, which has the per-substep plan alone: per substep every body's row, then every body's
// integration; bodies [nbodies][16] in place, out [nbodies][8] (the rows of the last substep) or NULL
int ds_step_bodies(int R, float uw, float period, int L, const float* depths, const float* pos, const float* vel, int iters, const float* hull,
                   int nverts, const int* tris, int ntris, float* bodies, const float* mass, int nbodies, const float* coeffs, float dt, int substeps,
                   float* out) {
    return hull_call(R, uw, period, L, depths, pos, vel, iters, hull, nverts, tris, ntris, coeffs, dt, substeps,
                     [&](const hull_order::Call& c, auto vertices) { hull_order::step_bodies(c, vertices, 0, bodies, mass, nbodies, out); });
}

}  // extern "C"
