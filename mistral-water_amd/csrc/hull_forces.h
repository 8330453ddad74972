// hull_forces.h -- buoyancy and drag on floating bodies (mw_ocean_hull_forces, include/mistral_water.h).
//
// One triangle mesh in body space (hull_xyz [nverts][3], triangles [ntris][3], (b - a) x (c - a) pointing out of the hull) shared by
// nbodies instances, each with a pose and velocities (bodies [nbodies][16] = p _ | q | v _ | w _).  Per instance vertex x = p + R(q) h
// the water is read where the world-mode surface query reads it (sq_locate, same frame and walk): height eta, depth d = eta - x.y and,
// with drag on, the water velocity u.  Per triangle the submerged part (the triangle clipped at d = 0 along its edges: 0, 1 or 2
// sub-triangles) takes the exact integral of the linear pressure rho g d,
//   F   = -rho g (D / 3) S,                                    S = (x1 - x0) x (x2 - x0) / 2, D = d0 + d1 + d2, r_i = x_i - p
//   tau = -(rho g / 12) (sum d_i r_i + D sum r_i) x S,         (int_T f g dA = A / 12 (sum f_i g_i + sum f_i sum g_i) for linear f, g)
// and, at its centroid c, linear and quadratic drag on v_rel = v + w x (c - p) - u(c).  On a closed hull over flat water the pressure
// terms sum to Archimedes exactly (divergence theorem: the waterline cap carries d = 0).
//
// Three launches, no atomics, every sum in a fixed order, so a body's row depends on nothing but its own inputs (bitwise the same
// alone or in a batch of any size):
//   k_hull_vertices   one lane per instance vertex: pose, sq_locate once, 32 B to the vertex slab (x y z d | ux uy uz residual)
//   k_hull_triangles  one 256-lane workgroup per (body, chunk of 256 triangles and 256 vertices): per-lane terms, then
//                     hull_chunk_partial: one partial row (7 sums, NaN-propagating max residual) per chunk
//   k_hull_reduce     one wave per body: hull_body_sum over its chunks, the row with the NaN rule applied (hull_row)
// The order of the sum is written once, in hull_wave_sum, hull_chunk_partial and hull_body_sum below; k_bodies_step (rigid_bodies.h)
// and the k_fleet_* kernels (fleet.h) call the same three, which is why their rows are these kernels' bit for bit.
//
// Everything but the __global__ wrappers and the three sums is MW_HD: tests/hull_forces_shim.cpp compiles the same functions with g++.
#pragma once
#include "surface_query.h"

namespace mw {

#define MW_HULL_CHUNK 256  // triangles (and vertices) per k_hull_triangles workgroup

// the chunks of a hull: every triangle and every vertex is in one
MW_HD int hull_chunks(int nverts, int ntris) { return ((ntris > nverts ? ntris : nverts) + MW_HULL_CHUNK - 1) / MW_HULL_CHUNK; }

// NaN-propagating max: once either side is NaN the result is NaN, whatever the order
MW_HD float hull_max(float a, float b) { return (a != a || b != b) ? NAN : fmaxf(a, b); }

MW_HD void hull_cross(const float a[3], const float b[3], float o[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// rotation matrix of the quaternion (qx, qy, qz, qw), normalised first; rows of R
MW_HD void hull_rotation(const float q[4], float R[9]) {
    const float inv = 1.f / sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    const float x = q[0] * inv, y = q[1] * inv, z = q[2] * inv, w = q[3] * inv;
    R[0] = 1.f - 2.f * (y * y + z * z); R[1] = 2.f * (x * y - z * w);       R[2] = 2.f * (x * z + y * w);
    R[3] = 2.f * (x * y + z * w);       R[4] = 1.f - 2.f * (x * x + z * z); R[5] = 2.f * (y * z - x * w);
    R[6] = 2.f * (x * z - y * w);       R[7] = 2.f * (y * z + x * w);       R[8] = 1.f - 2.f * (x * x + y * y);
}

// instance vertex x = p + R(q) h of body[16] (p _ q v _ w _)
MW_HD void hull_transform(const float body[16], const float h[3], float x[3]) {
    float R[9];
    hull_rotation(body + 4, R);
    for (int c = 0; c < 3; c++) x[c] = body[c] + (R[3 * c] * h[0] + R[3 * c + 1] * h[1] + R[3 * c + 2] * h[2]);
}

// The vertex step: one instance vertex -> slab[8] = (x, y, z, d, ux, uy, uz, residual).  eta, u and the residual come from the one
// sq_locate of the world-mode surface query at (x.x, x.z), accumulated as sq_query_point / sq_velocity_point accumulate them (eta is
// query_surface's py bit for bit).  vel == nullptr (drag off): u = 0.  A non-finite vertex has no answer: all eight are NaN.
// Mesh = SqTiled (a periodic handle): every vertex is located on the tiling on its own, so a hull may straddle a seam; x stays the world
// position, eta and u are those of the located point, the residual is taken in the base tile's frame.
template <typename Mesh>
MW_HD void hull_vertex(const Mesh& m, const float* vel, float vscale, int iters, const float body[16], const float h[3],
                       float slab[8]) {
    float x[3];
    hull_transform(body, h, x);
    const bool finite = fabsf(x[0]) <= 3.4e38f && fabsf(x[1]) <= 3.4e38f && fabsf(x[2]) <= 3.4e38f;
    if (!finite) {
        for (int k = 0; k < 8; k++) slab[k] = NAN;
        return;
    }
    sq_locate(m, MW_SQ_WORLD, x[0], x[2], iters, [&] { for (int k = 0; k < 8; k++) slab[k] = NAN; }, [&](const int v[3], const float w[3], const SqTile& t) {
        float eta = 0.f, u[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < 3; k++) eta += w[k] * m.vert[3 * v[k] + 1];
        if (vel)
            for (int k = 0; k < 3; k++)
                for (int c = 0; c < 3; c++) u[c] += w[k] * vel[3 * v[k] + c];
        slab[0] = x[0]; slab[1] = x[1]; slab[2] = x[2];
        slab[3] = eta - x[1];
        slab[4] = u[0] * vscale; slab[5] = u[1] * vscale; slab[6] = u[2] * vscale;
        slab[7] = sq_residual(m, v, w, t);
    });
}

// one corner of a (sub-)triangle: position, depth, water velocity
struct HullCorner {
    float x[3];
    float d;
    float u[3];
};

// the point where the edge from a wet corner (d > 0) to a dry one (d <= 0) meets d = 0: linear interpolation of position and water
// velocity, depth exactly 0.  The denominator is > 0, so the fraction is in (0, 1]; a dry corner at d = 0 is its own cut point.
MW_HD HullCorner hull_cut(const HullCorner& wet, const HullCorner& dry) {
    const float t = wet.d / (wet.d - dry.d);
    HullCorner c;
    for (int k = 0; k < 3; k++) {
        c.x[k] = wet.x[k] + t * (dry.x[k] - wet.x[k]);
        c.u[k] = wet.u[k] + t * (dry.u[k] - wet.u[k]);
    }
    c.d = 0.f;
    return c;
}

// Clips corners c0 c1 c2 (in the triangle's winding) at d = 0 and hands emit(s0, s1, s2) its 0, 1 or 2 submerged sub-triangles, of the
// same winding; returns their count.  A corner is wet for d > 0; corners at d = 0 are dry, so a triangle touching the waterline at a
// vertex or an edge adds nothing twice and no cut divides by zero.  Corners are selected by value, never by a run-time array index
// (which would put them in scratch).
template <typename Emit>
MW_HD int hull_clip(const HullCorner& c0, const HullCorner& c1, const HullCorner& c2, Emit emit) {
    const bool w0 = c0.d > 0.f, w1 = c1.d > 0.f, w2 = c2.d > 0.f;
    const int nwet = (int)w0 + (int)w1 + (int)w2;
    if (nwet == 0) return 0;
    if (nwet == 3) {
        emit(c0, c1, c2);
        return 1;
    }
    // rotate (a cyclic shift keeps the winding) so that the odd corner out comes first
    const int first = nwet == 1 ? (w0 ? 0 : w1 ? 1 : 2) : (!w0 ? 0 : !w1 ? 1 : 2);
    const HullCorner a = first == 0 ? c0 : first == 1 ? c1 : c2;
    const HullCorner b = first == 0 ? c1 : first == 1 ? c2 : c0;
    const HullCorner c = first == 0 ? c2 : first == 1 ? c0 : c1;
    if (nwet == 1) {  // a wet: the tip (a, ab, ac)
        emit(a, hull_cut(a, b), hull_cut(a, c));
        return 1;
    }
    // a dry, b and c wet: the quad (ab, b, c, ca) as (ab, b, c) and (ab, c, ca)
    const HullCorner ab = hull_cut(b, a), ca = hull_cut(c, a);
    emit(ab, b, c);
    emit(ab, c, ca);
    return 2;
}

// the coefficients of one call; rho_g = density * gravity, drag = (linear_drag > 0 || quadratic_drag > 0)
struct HullCoeffs {
    float rho_g, lin, quad;
    int drag;
};
// from the five coefficients of the ABI, k = (density, gravity, linear_drag, quadratic_drag, velocity_scale)
MW_HD void hull_coeffs(const float k[5], HullCoeffs* cf, float* g, float* vscale) {
    *cf = HullCoeffs{k[0] * k[1], k[2], k[3], (k[2] > 0.f || k[3] > 0.f) ? 1 : 0};
    *g = k[1];
    *vscale = k[4];
}

// pressure and drag of one submerged sub-triangle about p, added to acc[7] = (Fx, Fy, Fz, area, tx, ty, tz); body[16] as above
MW_HD void hull_subtriangle(const HullCorner& s0, const HullCorner& s1, const HullCorner& s2, const float body[16], const HullCoeffs& cf,
                            float acc[7]) {
    const float* p = body;
    const HullCorner* s[3] = {&s0, &s1, &s2};
    float e1[3], e2[3], S[3], r[3][3];
    for (int k = 0; k < 3; k++) {
        e1[k] = s[1]->x[k] - s[0]->x[k];
        e2[k] = s[2]->x[k] - s[0]->x[k];
        for (int i = 0; i < 3; i++) r[i][k] = s[i]->x[k] - p[k];
    }
    hull_cross(e1, e2, S);
    for (int k = 0; k < 3; k++) S[k] *= 0.5f;
    const float D = s0.d + s1.d + s2.d;
    // pressure: F = -rho g (D/3) S, tau = -(rho g / 12) (sum d_i r_i + D sum r_i) x S
    const float fp = -cf.rho_g * (D / 3.f);
    float M[3];
    for (int k = 0; k < 3; k++)
        M[k] = (s0.d * r[0][k] + s1.d * r[1][k] + s2.d * r[2][k]) + D * (r[0][k] + r[1][k] + r[2][k]);
    float tp[3];
    hull_cross(M, S, tp);
    const float tk = -cf.rho_g / 12.f;
    const float A = sqrtf(S[0] * S[0] + S[1] * S[1] + S[2] * S[2]);
    for (int k = 0; k < 3; k++) {
        acc[k] += fp * S[k];
        acc[4 + k] += tk * tp[k];
    }
    acc[3] += A;
    if (!cf.drag) return;
    // drag at the centroid c: v_rel = v + w x (c - p) - u(c)
    float rc[3], uc[3], wxr[3];
    for (int k = 0; k < 3; k++) {
        rc[k] = (r[0][k] + r[1][k] + r[2][k]) / 3.f;
        uc[k] = (s0.u[k] + s1.u[k] + s2.u[k]) / 3.f;
    }
    hull_cross(body + 12, rc, wxr);
    float vr[3], F[3];
    for (int k = 0; k < 3; k++) vr[k] = body[8 + k] + wxr[k] - uc[k];
    for (int k = 0; k < 3; k++) F[k] = -cf.lin * A * vr[k];
    if (A > 0.f) {  // quadratic drag on a face advancing into the water (v_rel . n > 0) only
        const float vn = (vr[0] * S[0] + vr[1] * S[1] + vr[2] * S[2]) / A;
        if (vn > 0.f) {
            const float q = -cf.quad * vn * vn;  // -quad A vn^2 n = -quad vn^2 S
            for (int k = 0; k < 3; k++) F[k] += q * S[k];
        }
    }
    float td[3];
    hull_cross(rc, F, td);
    for (int k = 0; k < 3; k++) {
        acc[k] += F[k];
        acc[4 + k] += td[k];
    }
}

// The triangle step: triangle (i0, i1, i2) of one body, its corners' vertex slabs vs [nverts][8] -> acc[7] += its terms.  Returns
// false for an index outside [0, nverts) (nothing is read then; the caller makes the row NaN).
MW_HD bool hull_triangle(const int idx[3], int nverts, const float* vs, const float body[16], const HullCoeffs& cf, float acc[7]) {
    HullCorner c[3];
    for (int k = 0; k < 3; k++) {
        if (!(idx[k] >= 0 && idx[k] < nverts)) return false;
    }
    for (int k = 0; k < 3; k++) {
        const float* s = vs + 8 * (size_t)idx[k];
        c[k].x[0] = s[0]; c[k].x[1] = s[1]; c[k].x[2] = s[2];
        c[k].d = s[3];
        c[k].u[0] = s[4]; c[k].u[1] = s[5]; c[k].u[2] = s[6];
    }
    hull_clip(c[0], c[1], c[2], [&](const HullCorner& s0, const HullCorner& s1, const HullCorner& s2) { hull_subtriangle(s0, s1, s2, body, cf, acc); });
    return true;
}

// the row of a body from its summed terms and max residual: out[8] = (F, area, tau, residual), all NaN when the residual is NaN
// (a vertex without an answer, or a bad index)
MW_HD void hull_row(const float acc[7], float res, float out[8]) {
    const bool bad = res != res;
    for (int k = 0; k < 3; k++) {
        out[k] = bad ? NAN : acc[k];
        out[4 + k] = bad ? NAN : acc[4 + k];
    }
    out[3] = bad ? NAN : acc[3];
    out[7] = res;
}

#if defined(__HIPCC__)
template <typename Mesh>
struct HullArgsT {
    Mesh m;
    const float* vel;  // per-vertex water velocity [R*R][3] (drag on), else nullptr
    float vscale;
    int iters;
    HullCoeffs cf;
    const float* hull;   // [nverts][3]
    const int* tris;     // [ntris][3]
    const float4* bodies;  // [nbodies][4] float4
    int nverts, ntris, nchunks;
    int64_t nbodies;
    float4* vslab;  // [nbodies * nverts][2]
    float4* part;   // [nbodies * nchunks][2]
    float4* out;    // [nbodies][2]
};
using HullArgs = HullArgsT<SqMesh>;
// the same call as the SqTiled instantiations of the kernels take it (surface_tiled.hip): the mesh read as the tiling by k_hull_vertices
// on a periodic handle, and read by no kernel after the slab (the note below)
inline HullArgsT<SqTiled> hull_args_tiled(const HullArgs& a) {
    return HullArgsT<SqTiled>{SqTiled{a.m}, a.vel, a.vscale, a.iters, a.cf, a.hull, a.tris, a.bodies, a.nverts, a.ntris, a.nchunks, a.nbodies,
                              a.vslab, a.part, a.out};
}

MW_HD void hull_load_body(const float4* b, float body[16]) {
    for (int k = 0; k < 4; k++) {
        const float4 v = b[k];
        body[4 * k] = v.x; body[4 * k + 1] = v.y; body[4 * k + 2] = v.z; body[4 * k + 3] = v.w;
    }
}
// an 8-float row (slab entry, partial, output, mass or wrench row) as two float4
MW_HD void hull_load_row(const float4* p, float r[8]) {
    const float4 a = p[0], b = p[1];
    r[0] = a.x; r[1] = a.y; r[2] = a.z; r[3] = a.w;
    r[4] = b.x; r[5] = b.y; r[6] = b.z; r[7] = b.w;
}
MW_HD void hull_store_row(float4* p, const float r[8]) {
    p[0] = make_float4(r[0], r[1], r[2], r[3]);
    p[1] = make_float4(r[4], r[5], r[6], r[7]);
}

// The ordered sum of a body's row, the one definition every kernel of hull_forces.h, rigid_bodies.h and fleet.h calls.
// The shuffle tree of one wave: lane 0 ends with the seven sums and the NaN-propagating max of the 64 lanes.
__device__ inline void hull_wave_sum(float acc[7], float& res) {
    for (int off = 32; off > 0; off >>= 1) {
        for (int k = 0; k < 7; k++) acc[k] += __shfl_down(acc[k], off, 64);
        res = hull_max(res, __shfl_down(res, off, 64));
    }
}
// The partial row of one chunk from the per-lane terms of a MW_HULL_CHUNK-lane workgroup: the tree of each wave, then thread 0 adds
// the waves in wave order and stores the row at dst (global memory or LDS).  The waves meet in 128 B of static LDS, free again on
// return; its rows are float4 pairs, so that each is written and read as two 16-byte accesses however this is inlined.
__device__ inline void hull_chunk_partial(float acc[7], float res, float4* dst) {
    __shared__ float4 red[MW_HULL_CHUNK / 64][2];
    const int l = threadIdx.x;
    hull_wave_sum(acc, res);
    if ((l & 63) == 0) {
        const float o[8] = {acc[0], acc[1], acc[2], acc[3], acc[4], acc[5], acc[6], res};
        hull_store_row(red[l >> 6], o);
    }
    __syncthreads();
    if (l == 0) {
        float o[8], r[8];
        hull_load_row(red[0], o);
        for (int w = 1; w < MW_HULL_CHUNK / 64; w++) {
            hull_load_row(red[w], r);
            for (int k = 0; k < 7; k++) o[k] += r[k];
            o[7] = hull_max(o[7], r[7]);
        }
        hull_store_row(dst, o);
    }
    __syncthreads();
}
// The sums of one body from its partials, rows first ... first + nchunks - 1 of part, by one wave: lane l takes chunks l, l + 64, ...
// in order, then the tree.  Lane 0 holds what hull_row takes.
__device__ inline void hull_body_sum(const float4* part, size_t first, int nchunks, int l, float acc[7], float& res) {
    for (int k = 0; k < 7; k++) acc[k] = 0.f;
    res = 0.f;
    for (int c = l; c < nchunks; c += 64) {
        float r[8];
        hull_load_row(part + 2 * (first + c), r);
        for (int k = 0; k < 7; k++) acc[k] += r[k];
        res = hull_max(res, r[7]);
    }
    hull_wave_sum(acc, res);
}
// The per-lane terms before these sums stay in the kernels: k_hull_triangles and k_fleet_triangles load the body only where
// t < ntris, the one-launch kernels hold it in registers, and one function for both would cost the first two a load or take a functor.

// One lane per instance vertex (n = nbodies * nverts < 2^31): the body's 64 B (shared by the lanes of a body: cache hits), the walk's
// gathers, two 16-byte stores.
template <typename Mesh>
__global__ __launch_bounds__(256) void k_hull_vertices(HullArgsT<Mesh> a) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.nbodies * a.nverts) return;
    const unsigned b = (unsigned)k / (unsigned)a.nverts;  // k < 2^31
    const int v = (int)((unsigned)k - b * (unsigned)a.nverts);
    float body[16], h[3], s[8];
    hull_load_body(a.bodies + 4 * (size_t)b, body);
    for (int c = 0; c < 3; c++) h[c] = a.hull[3 * (size_t)v + c];
    hull_vertex(a.m, a.vel, a.vscale, a.iters, body, h, s);
    hull_store_row(a.vslab + 2 * k, s);
}

// The kernels after the slab -- k_hull_triangles and k_hull_reduce below ("the rows") and k_bodies_integrate (rigid_bodies.h) -- read
// nothing of a.m: their Mesh parameter only names the translation unit, and with it the rounding, an instantiation is built in.  SqMesh
// is mistral_water.hip's, built with contraction and bit-pinned; SqTiled is surface_tiled.hip's, built without, and serves every call
// whose rows are the strict float32 of the g++ build whatever wrote the slab: a periodic handle (k_hull_vertices<SqTiled>) and draught
// on either handle (k_draught_vertices, water_column.hip).  One set of after-slab kernels per rounding mode; only the vertex phase varies.

// One 256-lane workgroup per (body, chunk): lane l takes triangle c*256 + l and the residual of vertex c*256 + l (every vertex is
// counted once, referenced or not); hull_chunk_partial reduces the 8 values.  Workgroups stride over the chunks (a 1-D grid of at most
// 2^20 workgroups); each chunk is done by one workgroup start to finish.
template <typename Mesh>
__global__ __launch_bounds__(256) void k_hull_triangles(HullArgsT<Mesh> a) {
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

// One wave per body: hull_body_sum, then lane 0 writes the row.  Waves stride over the bodies (a 1-D grid of at most 2^20 workgroups).
template <typename Mesh>
__global__ __launch_bounds__(256) void k_hull_reduce(HullArgsT<Mesh> a) {
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
#endif

}  // namespace mw
