// surface_tiled.hip -- the SqTiled instantiations of the surface services' kernels (surface_tiled.h), compiled without floating-point
// contraction.  The pragma stands after mw_math.h, which ends by setting its own, and before the headers whose MW_HD functions the
// kernels run: every multiply and add of the walk, the hull integrals and the integrator keeps its own rounding here.
#include <hip/hip_runtime.h>

#include "mw_host.h"  // AttrOnce
#include "mw_math.h"
#pragma clang fp contract(off)
#define MW_RC_NO_KERNELS  // k_raycast and k_rc_build_top are mistral_water.hip's
#define MW_STRICT_LINE_KERNELS  // k_moored_integrate and k_rigged_integrate stand here alone
#include "surface_tiled.h"
#include "raycast_tiled.h"

namespace mw {

static_assert(MW_RCT_MAX_REACH == MW_RC_MAX_REACH, "raycast_tiled.h and the ABI bound the reach alike");

hipError_t tiled_query_surface(dim3 grid, hipStream_t s, const SqMesh& m, int mode, int iters, const float2* xz, int64_t n, float4* out) {
    k_query_surface<<<grid, dim3(256), 0, s>>>(SqTiled{m}, mode, iters, xz, n, out);
    return hipGetLastError();
}

hipError_t tiled_query_velocity(dim3 grid, hipStream_t s, const SqMesh& m, const float* vel, int mode, int iters, const float2* xz, int64_t n,
                                float4* out) {
    k_query_velocity<<<grid, dim3(256), 0, s>>>(SqTiled{m}, vel, mode, iters, xz, n, out);
    return hipGetLastError();
}

hipError_t tiled_hull_vertices(dim3 grid, hipStream_t s, const HullArgs& a) {
    k_hull_vertices<<<grid, dim3(256), 0, s>>>(hull_args_tiled(a));
    return hipGetLastError();
}

hipError_t strict_hull_rows(dim3 triangles, dim3 reduce, hipStream_t s, const HullArgs& a) {
    const HullArgsT<SqTiled> t = hull_args_tiled(a);
    k_hull_triangles<<<triangles, dim3(MW_HULL_CHUNK), 0, s>>>(t);
    k_hull_reduce<<<reduce, dim3(256), 0, s>>>(t);
    return hipGetLastError();
}

hipError_t strict_bodies_integrate(dim3 grid, hipStream_t s, const BodiesArgs& a) {
    k_bodies_integrate<<<grid, dim3(256), 0, s>>>(bodies_args_tiled(a));
    return hipGetLastError();
}

hipError_t tiled_fleet_forces(dim3 vertices, dim3 triangles, dim3 reduce, hipStream_t s, const FleetArgs& a) {
    const FleetArgsT<SqTiled> t = fleet_args_tiled(a);
    k_fleet_vertices<<<vertices, dim3(256), 0, s>>>(t);
    k_fleet_triangles<<<triangles, dim3(MW_HULL_CHUNK), 0, s>>>(t);
    k_fleet_reduce<<<reduce, dim3(256), 0, s>>>(t);
    return hipGetLastError();
}

hipError_t tiled_fleet_integrate(dim3 grid, hipStream_t s, const FleetArgs& a) {
    if (a.wrench) k_fleet_integrate<SqTiled, true><<<grid, dim3(256), 0, s>>>(fleet_args_tiled(a));
    else k_fleet_integrate<SqTiled, false><<<grid, dim3(256), 0, s>>>(fleet_args_tiled(a));
    return hipGetLastError();
}

hipError_t tiled_fleet_step(dim3 grid, size_t lds, int lds_max, hipStream_t s, const FleetArgs& a, const float4* lines, int K,
                            float* tension) {
    static AttrOnce attr;
    const hipError_t e = attr.set(reinterpret_cast<const void*>(k_fleet_step<SqTiled>), lds_max);
    if (e != hipSuccess) return e;
    k_fleet_step<<<grid, dim3(MW_HULL_CHUNK), lds, s>>>(fleet_args_tiled(a), lines, tension, K);
    return hipGetLastError();
}

hipError_t strict_moored_integrate(dim3 grid, hipStream_t s, const MooredArgs& a) {
    k_moored_integrate<<<grid, dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t strict_rigged_integrate(dim3 grid, hipStream_t s, const RigArgs& a) {
    k_rigged_integrate<<<grid, dim3(256), 0, s>>>(a);
    return hipGetLastError();
}

hipError_t tiled_raycast_build_leaves(dim3 grid, hipStream_t s, const SqMesh& m, const RcTree& tr) {
    k_rc_build_leaves<<<grid, dim3(256), 0, s>>>(SqTiled{m}, tr);
    return hipGetLastError();
}

hipError_t tiled_raycast(dim3 grid, hipStream_t s, const SqMesh& m, const RcTree& tr, const float4* rays, int64_t n, int reach, float4* out,
                         int4* hit) {
    k_raycast_tiled<<<grid, dim3(256), 0, s>>>(m, tr, rays, n, reach, out, hit);
    return hipGetLastError();
}

}  // namespace mw
