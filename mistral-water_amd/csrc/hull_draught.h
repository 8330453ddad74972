// hull_draught.h -- draught: the hull family reads the water column below it (mw_ocean_set_draught, include/mistral_water.h;
// DESIGN.md section 7k).
//
// hull_vertex (hull_forces.h) gives an instance vertex the depth eta - y and the surface particle's velocity however deep it lies.
// With draught on the vertex step is hull_vertex_draught: the vertex is a world point of the column query (col_world_point,
// water_column.h), its depth is the point's rest depth -- the pressure there over rho g -- and its water velocity the column's, so the
// wave pressure under a hull of draught T falls off as e^{-kT} and the drag acts against the water down there.  In the air the column
// returns eta - y and no velocity, so a dry corner carries what it carries without draught and hull_cut meets d = 0 between a wet and a
// dry corner; below the deepest layer the rest depth continues hydrostatically.  Everything after the slab -- the clip, the integrals,
// the ordered sum, the integration -- is hull_forces.h's and rigid_bodies.h's, called and not copied: the functions and the kernels.
//
// Draught adds one kernel, k_draught_vertices (water_column.hip, built without floating-point contraction).  The slab it writes goes to
// the strict build of k_hull_triangles, k_hull_reduce and k_bodies_integrate that surface_tiled.hip already holds for the periodic
// handle (strict_hull_rows, strict_bodies_integrate): those kernels read no mesh, so the instantiation named SqTiled serves the one
// footprint as well (hull_forces.h).  The SqMesh instantiations, built with contraction and bit-pinned, are not touched, and no
// template is instantiated in two translation units.  Without contraction every draught row is what the g++ build of these functions
// computes (tests/draught_shim.cpp), bit for bit, on the one footprint and on the tiling alike.
#pragma once
#include "hull_forces.h"
#include "water_column.h"

namespace mw {

// The vertex step with draught: one instance vertex -> slab[8] = (x, y, z, rest depth, ux, uy, uz, residual), u = 0 with drag off.  A
// non-finite vertex or a column query without an answer: all eight are NaN.  The slab is written in one place, by value.
template <typename Mesh>
MW_HD void hull_vertex_draught(const Mesh& m, const ColTable& tb, int drag, float vscale, int iters, const float body[16], const float h[3],
                               float slab[8]) {
    float x[3];
    hull_transform(body, h, x);
    const bool finite = fabsf(x[0]) <= 3.4e38f && fabsf(x[1]) <= 3.4e38f && fabsf(x[2]) <= 3.4e38f;
    ColAnswer q{};
    if (finite) col_world_point(m, tb, x[0], x[1], x[2], iters, &q);
    const bool ok = finite && q.ok;
    const float u0 = drag ? q.a.u[0] : 0.f, u1 = drag ? q.a.u[1] : 0.f, u2 = drag ? q.a.u[2] : 0.f;
    const float row[8] = {x[0], x[1], x[2], q.rest_depth, u0 * vscale, u1 * vscale, u2 * vscale, q.residual};
    for (int k = 0; k < 8; k++) slab[k] = ok ? row[k] : NAN;
}

#if defined(__HIPCC__)
// what k_draught_vertices takes: the mesh (its vert is not read: every layer names its own), the layer table, and of the hull call the
// pose and vertex arrays and the slab
template <typename Mesh>
struct DraughtArgsT {
    Mesh m;
    ColTable tb;
    int drag;
    float vscale;
    int iters;
    const float* hull;     // [nverts][3]
    const float4* bodies;  // [nbodies][4] float4
    int nverts;
    int64_t nbodies;
    float4* vslab;         // [nbodies * nverts][2]
};

// how the host code (surface_services.inc) launches the vertex phase with draught on: k_draught_vertices on the grid gv of
// hull_reserve, a.m.period != 0 selecting its SqTiled instantiation; enqueues on s and returns hipGetLastError()
MW_INTERNAL hipError_t draught_vertices_launch(hipStream_t s, dim3 gv, const HullArgs& a, const ColTable& tb);
#endif

}  // namespace mw
