// rigid_bodies.h -- floating bodies: the substep chain of mw_ocean_step_bodies (include/mistral_water.h).
//
// nbodies instances of one hull (hull_forces.h: the same mesh, body layout and row) each with a mass row mass [nbodies][8] =
// m Ixx Iyy Izz Ixy Ixz Iyz 0 (the inertia tensor's entries about the centre of mass p, body axes), stepped by semi-implicit Euler with
// h = dt / substeps.  Per substep, in this order:
//   1. the hull-forces row (F, A, tau) at the current state, exactly as mw_ocean_hull_forces computes it
//   2. v <- v + h (F / m + (0, -g, 0))
//   3. w <- w + h I_w^-1 (tau - w x (I_w w)),   I_w = R I_b R^T, R = hull_rotation(q); evaluated in body axes:
//      w_b = R^T w, tau_b = R^T tau, w <- w + h R I_b^-1 (tau_b - w_b x (I_b w_b))  (the same quantity: R is orthonormal)
//   4. p <- p + h v
//   5. q <- normalize(q + (h / 2) (w, 0) (x) q)
// A NaN row leaves the body as it was at the start of that substep (and, the state being unchanged, every later substep of the call
// computes the same NaN row); an invalid mass row (m <= 0 or not finite, I_b not positive definite by its leading minors in f32)
// leaves the body unchanged with a NaN row.
//
// Two plans with the same bits (surface_services.inc: bodies_launch, switch MW_BODIES_PLAN):
//   per substep   hull_launch's three kernels, then k_bodies_integrate (one lane per body), once per substep
//   one launch    k_bodies_step: one workgroup per body runs every substep; the vertex slab (32 B per vertex), the per-chunk partial
//                 rows and the pose stay in LDS.  Its phases call what k_hull_vertices, k_hull_triangles and k_hull_reduce call
//                 (hull_vertex, hull_triangle, hull_chunk_partial, hull_body_sum, hull_row), so its rows are hull_launch's bit for
//                 bit.  Only workgroup barriers: no flags, no atomics, nothing between workgroups.
//                 k_bodies_step is instantiated for SqMesh alone, with contraction (mistral_water.hip).  It is the one kernel that
//                 cannot share its loop: built from a routine shared with k_fleet_step it lost its bits, because the compiler
//                 fused another operand.  Strict kernels can share it, and do: a periodic handle runs
//                 k_fleet_step (fleet.h), the same loop with the hull read from a one-hull table, where equal operations give
//                 equal bits.
//
// Everything but the __global__ wrappers is MW_HD: tests/bodies_shim.cpp compiles the same functions with g++.
#pragma once
#include "hull_forces.h"

namespace mw {

// the inverse of the symmetric I_b of a mass row (Ixx Iyy Izz Ixy Ixz Iyz at mass[1..6]) as (xx yy zz xy xz yz); returns det(I_b)
MW_HD float body_inverse_inertia(const float mass[8], float inv[6]) {
    const float xx = mass[1], yy = mass[2], zz = mass[3], xy = mass[4], xz = mass[5], yz = mass[6];
    const float c00 = yy * zz - yz * yz, c01 = xz * yz - xy * zz, c02 = xy * yz - xz * yy;
    const float c11 = xx * zz - xz * xz, c12 = xy * xz - xx * yz, c22 = xx * yy - xy * xy;
    const float det = xx * c00 + xy * c01 + xz * c02;
    const float r = 1.f / det;
    inv[0] = c00 * r; inv[1] = c11 * r; inv[2] = c22 * r;
    inv[3] = c01 * r; inv[4] = c02 * r; inv[5] = c12 * r;
    return det;
}

// a usable mass row: 0 < m finite, every entry finite, I_b positive definite by its leading minors (Ixx, Ixx Iyy - Ixy^2, det) in f32
MW_HD bool body_mass_valid(const float mass[8]) {
    if (!(mass[0] > 0.f && mass[0] <= 3.4e38f)) return false;
    for (int k = 1; k < 7; k++)
        if (!(fabsf(mass[k]) <= 3.4e38f)) return false;
    float inv[6];
    const float det = body_inverse_inertia(mass, inv);
    const float m2 = mass[1] * mass[2] - mass[4] * mass[4];
    return mass[1] > 0.f && m2 > 0.f && det > 0.f && det <= 3.4e38f;
}

// M x for the symmetric M = (xx yy zz xy xz yz)
MW_HD void body_sym_mul(const float M[6], const float x[3], float y[3]) {
    y[0] = M[0] * x[0] + M[3] * x[1] + M[4] * x[2];
    y[1] = M[3] * x[0] + M[1] * x[1] + M[5] * x[2];
    y[2] = M[4] * x[0] + M[5] * x[1] + M[2] * x[2];
}

// One substep (steps 2-5 above) of body[16] (p _ q v _ w _) under the row (F, A, tau, residual) of its current state; floats 3, 11 and
// 15 are not touched.  Returns false, changing nothing, when the row holds a NaN.  The mass row must be valid (body_mass_valid).
MW_HD bool body_integrate(float body[16], const float row[8], const float mass[8], float g, float h) {
    for (int k = 0; k < 8; k++)
        if (row[k] != row[k]) return false;
    float R[9], Ii[6];
    hull_rotation(body + 4, R);
    body_inverse_inertia(mass, Ii);
    const float Ib[6] = {mass[1], mass[2], mass[3], mass[4], mass[5], mass[6]};
    // 2. v <- v + h (F / m + (0, -g, 0))
    const float m = mass[0];
    const float a[3] = {row[0] / m, row[1] / m - g, row[2] / m};
    for (int k = 0; k < 3; k++) body[8 + k] = body[8 + k] + h * a[k];
    // 3. w <- w + h R I_b^-1 (tau_b - w_b x (I_b w_b)), in body axes (x_b = R^T x)
    float wb[3], tb[3];
    for (int k = 0; k < 3; k++) {
        wb[k] = R[k] * body[12] + R[3 + k] * body[13] + R[6 + k] * body[14];
        tb[k] = R[k] * row[4] + R[3 + k] * row[5] + R[6 + k] * row[6];
    }
    float Lb[3], gyro[3], rhs[3], dwb[3];
    body_sym_mul(Ib, wb, Lb);
    hull_cross(wb, Lb, gyro);
    for (int k = 0; k < 3; k++) rhs[k] = tb[k] - gyro[k];
    body_sym_mul(Ii, rhs, dwb);
    for (int k = 0; k < 3; k++) body[12 + k] = body[12 + k] + h * (R[3 * k] * dwb[0] + R[3 * k + 1] * dwb[1] + R[3 * k + 2] * dwb[2]);
    // 4. p <- p + h v
    for (int k = 0; k < 3; k++) body[k] = body[k] + h * body[8 + k];
    // 5. q <- normalize(q + (h / 2) (w, 0) (x) q):  (w, 0) (x) (qv, qw) = (qw w + w x qv, -w . qv)
    const float hh = 0.5f * h;
    const float* w = body + 12;
    float* q = body + 4;
    float wxq[3];
    hull_cross(w, q, wxq);
    float n[4];
    for (int k = 0; k < 3; k++) n[k] = q[k] + hh * (q[3] * w[k] + wxq[k]);
    n[3] = q[3] - hh * (w[0] * q[0] + w[1] * q[1] + w[2] * q[2]);
    const float inv = 1.f / sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2] + n[3] * n[3]);
    for (int k = 0; k < 4; k++) q[k] = n[k] * inv;
    return true;
}

// The pushed row: a body under its water row and a wrench from outside the water -- the external wrench of a fleet call (fleet.h) or
// the wrench of the body's lines (rigging.h).  It stands here, below the integrator, because every header built on this one pushes it.
// a usable wrench row (Fx Fy Fz _ tx ty tz _): the six entries finite
MW_HD bool fleet_wrench_valid(const float wrench[8]) {
    for (int k = 0; k < 3; k++)
        if (!(fabsf(wrench[k]) <= 3.4e38f && fabsf(wrench[4 + k]) <= 3.4e38f)) return false;
    return true;
}
// The row steps 2 and 3 of the integrator see: the water row, and when wrench != nullptr the external force and torque added to it,
// F[k] + wrench[k] and tau[k] + wrench[4 + k], one float32 add each.  wrench == nullptr: the water row itself, no addition.
MW_HD void fleet_pushed_row(const float row[8], const float* wrench, float r[8]) {
    for (int k = 0; k < 8; k++) r[k] = row[k];
    if (!wrench) return;
    for (int k = 0; k < 3; k++) {
        r[k] = row[k] + wrench[k];
        r[4 + k] = row[4 + k] + wrench[4 + k];
    }
}
// One substep of a body under its water row and its wrench (nullptr: none, and then this is body_integrate on the row).
MW_HD bool fleet_integrate(float body[16], const float row[8], const float mass[8], const float* wrench, float g, float h) {
    float r[8];
    fleet_pushed_row(row, wrench, r);
    return body_integrate(body, r, mass, g, h);
}

// LDS of k_bodies_step beyond its static arrays: the vertex slab and the chunk partials, 32 B each
inline size_t bodies_step_lds(int nverts, int nchunks) { return ((size_t)nverts + (size_t)nchunks) * 8 * sizeof(float); }
// dynamic LDS k_bodies_step may take: one MI355X CU's 160 KiB less 1 KiB for its static arrays
#define MW_BODIES_LDS_MAX (160 * 1024 - 1024)

#if defined(__HIPCC__)
template <typename Mesh>
struct BodiesArgsT {
    HullArgsT<Mesh> h;            // the hull-forces arguments of the call (h.bodies = bodies, h.out = the per-substep rows)
    float4* bodies;        // [nbodies][4] float4, updated in place
    const float4* mass;    // [nbodies][2]
    const float4* rows;    // per-substep plan: hull_launch's rows of this substep [nbodies][2]
    float4* out;           // [nbodies][2] or nullptr: the row of the last substep
    float g, dt;           // gravity, h = dt / substeps
    int substeps;
    int last;              // k_bodies_integrate: this is the call's last substep (write out)
};
using BodiesArgs = BodiesArgsT<SqMesh>;
inline BodiesArgsT<SqTiled> bodies_args_tiled(const BodiesArgs& a) {
    return BodiesArgsT<SqTiled>{hull_args_tiled(a.h), a.bodies, a.mass, a.rows, a.out, a.g, a.dt, a.substeps, a.last};
}

// Per-substep plan, after hull_launch: one lane per body integrates its row; the last substep also writes out.
template <typename Mesh>
__global__ __launch_bounds__(256) void k_bodies_integrate(BodiesArgsT<Mesh> a) {
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

// One-launch plan: one 256-lane workgroup per body runs every substep.  Per substep: the vertex phase (k_hull_vertices per lane, into
// the LDS slab), the triangle phase (k_hull_triangles per chunk, in chunk order, into the LDS partials), the row (k_hull_reduce) in
// wave 0 and, in lane 0, the integration; the new pose goes to every lane through LDS.
template <typename Mesh>
__global__ __launch_bounds__(MW_HULL_CHUNK) void k_bodies_step(BodiesArgsT<Mesh> a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float pose[16];
    __shared__ int stop;
    const HullArgsT<Mesh>& ha = a.h;
    float4* slab = reinterpret_cast<float4*>(smem);  // [nverts][2]
    float4* part = slab + 2 * (size_t)ha.nverts;     // [nchunks][2]
    const float* vs = reinterpret_cast<const float*>(slab);
    const int l = threadIdx.x;
    const int64_t b = blockIdx.x;
    float body[16], mass[8], row[8];
    hull_load_body(a.bodies + 4 * b, body);
    hull_load_row(a.mass + 2 * b, mass);
    if (!body_mass_valid(mass)) {  // uniform over the workgroup
        for (int k = 0; k < 8; k++) row[k] = NAN;
        if (l == 0 && a.out) hull_store_row(a.out + 2 * b, row);
        return;
    }
    for (int s = 0; s < a.substeps; s++) {
        // vertices (k_hull_vertices)
        for (int v = l; v < ha.nverts; v += MW_HULL_CHUNK) {
            float h[3], sl[8];
            for (int c = 0; c < 3; c++) h[c] = ha.hull[3 * (size_t)v + c];
            hull_vertex(ha.m, ha.vel, ha.vscale, ha.iters, body, h, sl);
            hull_store_row(slab + 2 * v, sl);
        }
        __syncthreads();
        // triangles (k_hull_triangles), chunk by chunk
        for (int c = 0; c < ha.nchunks; c++) {
            float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            float res = 0.f;
            const int t = c * MW_HULL_CHUNK + l;
            if (t < ha.ntris) {
                const int idx[3] = {ha.tris[3 * (size_t)t], ha.tris[3 * (size_t)t + 1], ha.tris[3 * (size_t)t + 2]};
                if (!hull_triangle(idx, ha.nverts, vs, body, ha.cf, acc)) res = NAN;
            }
            if (t < ha.nverts) res = hull_max(res, vs[8 * (size_t)t + 7]);
            hull_chunk_partial(acc, res, part + 2 * c);
        }
        // the row (k_hull_reduce) and the integration, in wave 0
        if (l < 64) {
            float acc[7], res;
            hull_body_sum(part, 0, ha.nchunks, l, acc, res);
            if (l == 0) {
                hull_row(acc, res, row);
                const bool ok = body_integrate(body, row, mass, a.g, a.dt);
                for (int k = 0; k < 16; k++) pose[k] = body[k];
                stop = ok ? 0 : 1;
            }
        }
        __syncthreads();
        for (int k = 0; k < 16; k++) body[k] = pose[k];
        if (stop) break;  // a NaN row: the state stays, and so would every later row
        __syncthreads();  // pose and stop are written again by the next substep
    }
    if (l == 0) {
        for (int k = 0; k < 4; k++) a.bodies[4 * b + k] = make_float4(body[4 * k], body[4 * k + 1], body[4 * k + 2], body[4 * k + 3]);
        if (a.out) hull_store_row(a.out + 2 * b, row);
    }
}
#endif

}  // namespace mw
