// surface_tiled.h -- how the host code launches the SqTiled instantiations of the surface services' kernels (a periodic handle,
// mw_ocean_set_periodic).  They are instantiated in a translation unit of their own, surface_tiled.hip, which compiles the MW_HD
// functions of surface_query.h, hull_forces.h and rigid_bodies.h without floating-point contraction: the tiled services are the
// strict float32 the g++ build of the same functions computes (tests/periodic_shim.cpp), bit for bit, as raycast.h is.  The SqMesh
// instantiations stay in mistral_water.hip, compiled as they always were, so a handle with the switch off keeps its bits.
// The tiled raycast (raycast_tiled.h, mw_ocean_raycast_tiled) has its kernels here for the same reason -- k_raycast_tiled and the SqTiled
// instantiation of raycast.h's k_rc_build_leaves: sq_shift, sq_reduce and the column planes of its walk must round as the g++ build
// rounds them (tests/raycast_tiled_shim.cpp).
// The kernels after the vertex slab (k_hull_triangles, k_hull_reduce, k_bodies_integrate, k_moored_integrate, k_rigged_integrate) do not read the mesh
// (hull_forces.h), so their
// instantiations here are the library's strict build of them: strict_hull_rows and strict_bodies_integrate serve a periodic handle and,
// on either handle, draught (hull_draught.h), whose own vertex kernel stands in water_column.hip.
//
// Each function enqueues on `s` with the grids the caller worked out (surface_services.inc: the same as for SqMesh) and returns
// hipGetLastError().  Internal to the library: hidden from its exported symbols.
#pragma once
#include "rigid_bodies.h"
#include "fleet.h"
#include "moorings.h"
#include "rigging.h"
#include "raycast.h"  // RcTree, k_rc_build_leaves

namespace mw {
#define MW_INTERNAL __attribute__((visibility("hidden")))
MW_INTERNAL hipError_t tiled_query_surface(dim3 grid, hipStream_t s, const SqMesh& m, int mode, int iters, const float2* xz, int64_t n, float4* out);
MW_INTERNAL hipError_t tiled_query_velocity(dim3 grid, hipStream_t s, const SqMesh& m, const float* vel, int mode, int iters, const float2* xz,
                                            int64_t n, float4* out);
// k_hull_vertices on the tiling: the vertex phase of a periodic handle without draught
MW_INTERNAL hipError_t tiled_hull_vertices(dim3 grid, hipStream_t s, const HullArgs& a);
// the strict build of the kernels after the slab, whichever vertex kernel wrote it: k_hull_triangles then k_hull_reduce on their two
// grids (the rows into a.out), and k_bodies_integrate
MW_INTERNAL hipError_t strict_hull_rows(dim3 triangles, dim3 reduce, hipStream_t s, const HullArgs& a);
MW_INTERNAL hipError_t strict_bodies_integrate(dim3 grid, hipStream_t s, const BodiesArgs& a);
// the fleet kernels (fleet.h): k_fleet_vertices, k_fleet_triangles, k_fleet_reduce on their three grids; k_fleet_integrate
MW_INTERNAL hipError_t tiled_fleet_forces(dim3 vertices, dim3 triangles, dim3 reduce, hipStream_t s, const FleetArgs& a);
MW_INTERNAL hipError_t tiled_fleet_integrate(dim3 grid, hipStream_t s, const FleetArgs& a);
// k_fleet_step, the one one-launch kernel of this translation unit (step fleet, and on a one-hull table step bodies and step moored;
// k_bodies_step is instantiated for SqMesh alone, in mistral_water.hip): `lds` bytes of dynamic LDS, at most lds_max (set as the
// kernel's attribute once per device); lines [total_bodies][K][3] and tension, K == 0: no lines
MW_INTERNAL hipError_t tiled_fleet_step(dim3 grid, size_t lds, int lds_max, hipStream_t s, const FleetArgs& a, const float4* lines, int K,
                                        float* tension);
// the per-substep line integrators, which read no mesh and serve every handle, after the rows of the substep: k_moored_integrate
// (moorings.h) and k_rigged_integrate (rigging.h)
MW_INTERNAL hipError_t strict_moored_integrate(dim3 grid, hipStream_t s, const MooredArgs& a);
MW_INTERNAL hipError_t strict_rigged_integrate(dim3 grid, hipStream_t s, const RigArgs& a);
// k_rc_build_leaves<SqTiled>: the leaf boxes of one tile and the levels above them up to D - 4 (k_rc_build_top, launched by the caller, does the
// rest); k_raycast_tiled: one lane per ray.  m.period is the tiling's P.
MW_INTERNAL hipError_t tiled_raycast_build_leaves(dim3 grid, hipStream_t s, const SqMesh& m, const RcTree& tr);
MW_INTERNAL hipError_t tiled_raycast(dim3 grid, hipStream_t s, const SqMesh& m, const RcTree& tr, const float4* rays, int64_t n, int reach,
                                     float4* out, int4* hit);
}  // namespace mw
