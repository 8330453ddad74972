// surface_query.h -- height, normal and whitecap of the displaced mesh at arbitrary horizontal positions
// (mw_ocean_query_surface, include/mistral_water.h).
//
// The surface is the triangle mesh the library hands out: vertex (i, j) of the R x R grid at i*R + j (i along x, j along z),
// each rest-grid cell (i, j) split along the diagonal (i, j+1)-(i+1, j) of the index buffer of S/FFTMesh.cs:118-131
// (rest_mesh_element): the lower triangle (i,j) (i,j+1) (i+1,j) and the upper triangle (i+1,j) (i,j+1) (i+1,j+1).  Inside a
// triangle everything is interpolated barycentrically in rest-plane coordinates, the normal is normalised afterwards.
//
// Rest mode: (x, z) is a rest-plane point, one triangle lookup.  World mode (buoyancy): find the rest point u whose
// displaced horizontal position is (x, z).  The iteration u <- (x, z) - D(u) walks the rest plane; at every visited point the map
// of its triangle is affine, so one exact 2 x 2 solve there gives the answer as soon as the solution lies inside that triangle
// (early exit).  The plain step contracts only by the largest eigenvalue of dD/du, which tends to 1 at the fold limit (8 steps
// leave 9 % of the points of a 128^2 synthetic mesh at 0.99 of the limit unresolved: tests/test_surface_query_cpu.py::
// test_preconditioned_walk_resolves_what_the_plain_iteration_leaves prints the figures); the walk therefore takes the step that
// solve names (the plain step times the inverse of the triangle's map: a Newton step of the piecewise-affine map), capped at
// MW_SQ_MAX_STEP cells, and the plain step only in folded triangles.  When no visited triangle contains its own solution (the mesh folds over itself, or the query is
// off the displaced footprint) the visited point with the smallest residual is returned: a point on the mesh and its honest
// distance |displaced(u).xz - (x, z)|.
//
// The tiled surface (mw_ocean_set_periodic): an FFTMesh frame on a grid with N * unit_width == length repeats with
// period P = N * unit_width, and SqTiled reads the same arrays as that infinite tiling.  Grid line g = k*N + a (floor division) rests at
// rest_coord(a) + k*P, vertex (gi, gj) is vertex (ai, aj) of the frame displaced by (ki*P, 0, kj*P), and every integer cell exists --
// cell a = N-1, between the last grid line and the next tile's first, is the seam.  A query is first reduced to the base tile
// ([rest(0), rest(0) + P] on both axes), located there by the same code with the wrapped forms of the cell lookup and the corner gather
// and no clamp, and its tile offset is added to the position once at the end: the answer depends on the reduced point and the tile
// indices alone, so its precision does not degrade with the distance from the origin.  The mesh TYPE selects the form at compile time:
// SqMesh instantiates what it always did.
//
// Everything but the __global__ wrapper is MW_HD: tests/surface_query_shim.cpp and tests/periodic_shim.cpp compile the same functions
// with g++.
#pragma once
#include <type_traits>

#include "mw_math.h"

namespace mw {

#define MW_SQ_REST 0
#define MW_SQ_WORLD 1
#define MW_SQ_DEFAULT_ITERS 8
#define MW_SQ_MAX_ITERS 64
#define MW_SQ_INSIDE_TOL 1e-5f  // barycentric slack of the in-triangle test (a solution on a shared edge belongs to both sides)
// longest step of the walk, in cells, and whether steps are preconditioned (0: the plain fixed-point step everywhere).  Both are
// compile-time only so that tests/test_surface_query_cpu.py::test_preconditioned_walk_resolves_what_the_plain_iteration_leaves can
// build the walks it compares; the library is always built with the defaults.
#ifndef MW_SQ_MAX_STEP
#define MW_SQ_MAX_STEP 4.f
#endif
#ifndef MW_SQ_PRECONDITION
#define MW_SQ_PRECONDITION 1
#endif

// the vertex arrays of one frame (device pointers on the GPU, host pointers in the shim)
struct SqMesh {
    const float* vert;   // [R*R][3] displaced positions
    const float* norm;   // [R*R][3] normals
    const float* white;  // [R*R][wstride], whitecap in channel 0 (FFTMesh colours: RGBA, stride 4; OceanRenderer: stride 1)
    int R;
    int wstride;
    float unit_width;
    float period;  // 0: the one footprint.  P = R * unit_width: the frame tiles with this period (set only where it does, query_prepare)
    static constexpr bool tiled = false;
};
// the same arrays read as the infinite tiling of the frame (period != 0)
struct SqTiled : SqMesh {
    static constexpr bool tiled = true;
};
#define MW_SQ_MAX_TILE 1048576.f  // queries further than 2^20 tiles from the base tile have no answer

// Where a located point sits: the query in the frame it was located in (SqMesh: the query itself; SqTiled: reduced to the base tile,
// kx and kz tiles away) and the tile (ki[c], kj[c]) that corner c of its triangle comes from.  SqMesh reads qx and qz only.
struct SqTile {
    float qx, qz;
    int kx, kz;
    int ki[3], kj[3];
};

// cell of one rest axis that holds x (x inside [rest_coord(0), rest_coord(R-1)]) and the fraction along it, measured between the
// cell's own rest coordinates so that a query at a vertex's rest coordinate gets a fraction of exactly 0 or 1
MW_HD int sq_cell(int R, float uw, float x, float* frac) {
    const float x0 = rest_coord(R, uw, 0);
    const float c = fminf(fmaxf(floorf((x - x0) / uw), 0.f), (float)(R - 2));  // NaN-safe: fmaxf(NaN, 0) = 0
    int i = (int)c;
    float a = rest_coord(R, uw, i), b = rest_coord(R, uw, i + 1);
    if (x < a && i > 0) {
        i--; b = a; a = rest_coord(R, uw, i);
    } else if (x > b && i < R - 2) {
        i++; a = b; b = rest_coord(R, uw, i + 1);
    }
    *frac = (x - a) / (b - a);
    return i;
}

// ---- the tiled forms ----
// x displaced by k periods; k = 0 leaves the bits of x alone
MW_HD float sq_shift(float x, int k, float P) { return k ? x + (float)k * P : x; }
// grid line g of the tiling = tile *k, line a of the frame (floor division, 0 <= a < N)
MW_HD int sq_wrap(int N, int g, int* k) {
    int q = g / N, a = g - q * N;
    if (a < 0) { a += N; q--; }
    *k = q;
    return a;
}
MW_HD float sq_tiled_rest(int N, float uw, float P, int g) {
    int k;
    const int a = sq_wrap(N, g, &k);
    return sq_shift(rest_coord(N, uw, a), k, P);
}
// x = xr + k*P with xr in the base tile [rest(0), rest(0) + P]; false for a non-finite x and for |k| > MW_SQ_MAX_TILE
MW_HD bool sq_reduce(int N, float uw, float P, float x, int* k, float* xr) {
    const float x0 = rest_coord(N, uw, 0);
    float kf = floorf((x - x0) / P);
    if (!(fabsf(kf) <= MW_SQ_MAX_TILE + 1.f)) return false;  // NaN and inf end here
    float r = x - kf * P;
    if (r < x0) {  // the quotient rounded across a tile boundary
        kf -= 1.f; r = x - kf * P;
    } else if (r > x0 + P) {
        kf += 1.f; r = x - kf * P;
    }
    if (fabsf(kf) > MW_SQ_MAX_TILE) return false;
    *k = (int)kf;
    *xr = r;
    return true;
}
// sq_cell on the tiling: any integer cell g, its ends at sq_tiled_rest(g) and sq_tiled_rest(g + 1).  On the base footprint it is
// sq_cell itself, so that a point there gets the very cell and fraction the one mesh gives it.
MW_HD int sq_cell_tiled(int N, float uw, float P, float x, float* frac) {
    const float x0 = rest_coord(N, uw, 0);
    if (x >= x0 && x <= rest_coord(N, uw, N - 1)) return sq_cell(N, uw, x, frac);
    const float c = fminf(fmaxf(floorf((x - x0) / uw), -1e9f), 1e9f);  // NaN-safe, and g +- 2 stays an int
    int g = (int)c;
    float a = sq_tiled_rest(N, uw, P, g), b = sq_tiled_rest(N, uw, P, g + 1);
    if (x < a) {
        g--; b = a; a = sq_tiled_rest(N, uw, P, g);
    } else if (x > b) {
        g++; a = b; b = sq_tiled_rest(N, uw, P, g + 1);
    }
    *frac = (x - a) / (b - a);
    return g;
}

// the triangle of cell (i, j) that holds local rest coordinates (fa, fb) and the barycentric weights of its corners.  Exact at the
// corners: a weight is 0 or 1 there, so a vertex's own rest position reproduces the vertex bit for bit.
MW_HD bool sq_upper(float fa, float fb) { return fa + fb > 1.f; }
MW_HD void sq_triangle(int R, int i, int j, bool upper, float fa, float fb, int v[3], float w[3]) {
    const int c00 = i * R + j;
    if (!upper) {
        v[0] = c00; v[1] = c00 + R; v[2] = c00 + 1;  // (i,j) (i+1,j) (i,j+1)
        w[0] = 1.f - fa - fb; w[1] = fa; w[2] = fb;
    } else {
        v[0] = c00 + R + 1; v[1] = c00 + R; v[2] = c00 + 1;  // (i+1,j+1) (i+1,j) (i,j+1)
        w[0] = fa + fb - 1.f; w[1] = 1.f - fb; w[2] = 1.f - fa;
    }
}

// sq_triangle on the tiling: cell (gi, gj) of the integer grid, the corners' indices wrapped into the frame and their tiles into t
MW_HD void sq_triangle_tiled(int N, int gi, int gj, bool upper, float fa, float fb, int v[3], float w[3], SqTile* t) {
    int ki0, ki1, kj0, kj1;
    const int i0 = sq_wrap(N, gi, &ki0) * N, i1 = sq_wrap(N, gi + 1, &ki1) * N;
    const int j0 = sq_wrap(N, gj, &kj0), j1 = sq_wrap(N, gj + 1, &kj1);
    if (!upper) {
        v[0] = i0 + j0; v[1] = i1 + j0; v[2] = i0 + j1;
        t->ki[0] = ki0; t->ki[1] = ki1; t->ki[2] = ki0;
        t->kj[0] = kj0; t->kj[1] = kj0; t->kj[2] = kj1;
        w[0] = 1.f - fa - fb; w[1] = fa; w[2] = fb;
    } else {
        v[0] = i1 + j1; v[1] = i1 + j0; v[2] = i0 + j1;
        t->ki[0] = ki1; t->ki[1] = ki1; t->ki[2] = ki0;
        t->kj[0] = kj1; t->kj[1] = kj0; t->kj[2] = kj1;
        w[0] = fa + fb - 1.f; w[1] = 1.f - fb; w[2] = 1.f - fa;
    }
}

// ---- what sq_locate and its callers read through the mesh type ----
template <typename Mesh>
MW_HD int sq_cell_of(const Mesh& m, float x, float* frac) {
    if constexpr (Mesh::tiled) return sq_cell_tiled(m.R, m.unit_width, m.period, x, frac);
    else return sq_cell(m.R, m.unit_width, x, frac);
}
template <typename Mesh>
MW_HD void sq_triangle_of(const Mesh& m, int i, int j, bool upper, float fa, float fb, int v[3], float w[3], SqTile* t) {
    if constexpr (Mesh::tiled) sq_triangle_tiled(m.R, i, j, upper, fa, fb, v, w, t);
    else sq_triangle(m.R, i, j, upper, fa, fb, v, w);
}
// horizontal position of corner c (vertex v) of a located triangle, in the frame of t
template <typename Mesh>
MW_HD float sq_corner_x(const Mesh& m, const SqTile& t, int v, int c) {
    if constexpr (Mesh::tiled) return sq_shift(m.vert[3 * v], t.ki[c], m.period);
    else return m.vert[3 * v];
}
template <typename Mesh>
MW_HD float sq_corner_z(const Mesh& m, const SqTile& t, int v, int c) {
    if constexpr (Mesh::tiled) return sq_shift(m.vert[3 * v + 2], t.kj[c], m.period);
    else return m.vert[3 * v + 2];
}

// The triangle's displaced horizontal map is affine in the cell's local rest coordinates: P(fa, fb) = O + fa ea + fb eb, corner
// positions p0 p1 p2 in the order of sq_triangle.  Solves P(sa, sb) = (qx, qz) and returns the map's determinant: > 0 where the
// triangle keeps its rest orientation, < 0 where the mesh folded it over, 0 (inf / NaN solution) where it collapsed.
MW_HD float sq_affine_solve(bool upper, const float px[3], const float pz[3], float qx, float qz, float* sa, float* sb) {
    float ox, oz, ax, az, bx, bz;
    if (!upper) {  // p0 + fa (p1 - p0) + fb (p2 - p0)
        ox = px[0]; oz = pz[0];
        ax = px[1] - px[0]; az = pz[1] - pz[0];
        bx = px[2] - px[0]; bz = pz[2] - pz[0];
    } else {       // (p1 + p2 - p0) + fa (p0 - p2) + fb (p0 - p1)
        ox = px[1] + px[2] - px[0]; oz = pz[1] + pz[2] - pz[0];
        ax = px[0] - px[2]; az = pz[0] - pz[2];
        bx = px[0] - px[1]; bz = pz[0] - pz[1];
    }
    const float rx = qx - ox, rz = qz - oz;
    const float det = ax * bz - bx * az;
    *sa = (rx * bz - bx * rz) / det;
    *sb = (ax * rz - rx * az) / det;
    return det;
}
// local coordinates inside the triangle (with MW_SQ_INSIDE_TOL of slack; false for NaN)
MW_HD bool sq_inside(bool upper, float sa, float sb) {
    const float t = MW_SQ_INSIDE_TOL;
    return !upper ? (sa >= -t && sb >= -t && sa + sb <= 1.f + t) : (sa <= 1.f + t && sb <= 1.f + t && sa + sb >= 1.f - t);
}

// The rest point a query resolves to: rest mode one lookup, world mode the walk.  Where the query has an answer, `found` receives the
// corners v and barycentric weights w of its triangle and the frame t they are in; where it has none -- a rest point off the footprint, a
// non-finite world point, on the tiling a point more than MW_SQ_MAX_TILE tiles out -- `miss` runs instead.  The surface query
// (sq_query_point) and the velocity query (sq_velocity_point) both locate here, so they resolve every point identically.
// SqTiled: the query is reduced to the base tile first, (ux, uz) and the cells range over the whole tiling in that frame, nothing clamps.
template <typename Mesh, typename Miss, typename Found>
MW_HD void sq_locate(const Mesh& m, int mode, float qx, float qz, int iters, Miss miss, Found found) {
    const int R = m.R;
    const float lo = fminf(rest_coord(R, m.unit_width, 0), rest_coord(R, m.unit_width, R - 1));
    const float hi = fmaxf(rest_coord(R, m.unit_width, 0), rest_coord(R, m.unit_width, R - 1));
    const bool rest = mode == MW_SQ_REST;
    SqTile t;  // kx, kz: sq_reduce; ki, kj: sq_triangle_tiled; qx, qz: below, once the walk is over
    bool ok;
    if constexpr (Mesh::tiled) {
        ok = sq_reduce(R, m.unit_width, m.period, qx, &t.kx, &qx) && sq_reduce(R, m.unit_width, m.period, qz, &t.kz, &qz);
    } else {
        // rest mode: the point must lie on the footprint; world mode: a finite point (the walk stays on the footprint by clamping)
        ok = rest ? (qx >= lo && qx <= hi && qz >= lo && qz <= hi) : (fabsf(qx) <= 3.4e38f && fabsf(qz) <= 3.4e38f);
    }
    if (!ok) {
        miss();
        return;
    }
    float ux = qx, uz = qz;
    if constexpr (!Mesh::tiled) { ux = fminf(fmaxf(qx, lo), hi); uz = fminf(fmaxf(qz, lo), hi); }
    int ci, cj;
    float fa, fb;
    ci = sq_cell_of(m, ux, &fa);
    cj = sq_cell_of(m, uz, &fb);
    bool up = sq_upper(fa, fb);
    if (!rest) {
        // the walk: (ci, cj, up, fa, fb) always names the best point so far; (ti, tj, tu, ta, tb) the point being visited
        float best = INFINITY;
        int ti = ci, tj = cj;
        bool tu = up;
        float ta = fa, tb = fb;
        for (int it = 0;; it++) {
            int v[3];
            float w[3], px[3], pz[3];
            sq_triangle_of(m, ti, tj, tu, ta, tb, v, w, &t);
            for (int k = 0; k < 3; k++) { px[k] = sq_corner_x(m, t, v[k], k); pz[k] = sq_corner_z(m, t, v[k], k); }
            float sa, sb;
            const float det = sq_affine_solve(tu, px, pz, qx, qz, &sa, &sb);
            if (sq_inside(tu, sa, sb)) {  // the preimage is in this triangle: the exact answer
                ci = ti; cj = tj; up = tu;
                fa = fminf(fmaxf(sa, 0.f), 1.f);
                fb = fminf(fmaxf(sb, 0.f), 1.f);
                break;
            }
            const float ex = w[0] * px[0] + w[1] * px[1] + w[2] * px[2] - qx, ez = w[0] * pz[0] + w[1] * pz[1] + w[2] * pz[2] - qz;
            const float r = ex * ex + ez * ez;
            if (r < best) { best = r; ci = ti; cj = tj; up = tu; fa = ta; fb = tb; }
            if (it >= iters) break;
            // next point: u <- q - D(u) = u - (P(u) - q), the step preconditioned by the inverse of this triangle's map (a Newton step
            // of the piecewise-affine P: the point its affine solve names) where the triangle is not folded, at most MW_SQ_MAX_STEP
            // cells long; the plain step in a folded or collapsed triangle
            float da = sa - ta, db = sb - tb;
            const float len = fmaxf(fabsf(da), fabsf(db));
            if (MW_SQ_PRECONDITION && det > 0.f && len <= 1e30f) {
                const float k = len > MW_SQ_MAX_STEP ? MW_SQ_MAX_STEP / len : 1.f;
                ux += da * k * m.unit_width;
                uz += db * k * m.unit_width;
            } else {
                ux -= ex;
                uz -= ez;
            }
            if constexpr (!Mesh::tiled) {
                ux = fminf(fmaxf(ux, lo), hi);
                uz = fminf(fmaxf(uz, lo), hi);
            }
            ti = sq_cell_of(m, ux, &ta);
            tj = sq_cell_of(m, uz, &tb);
            tu = sq_upper(ta, tb);
        }
    }
    int v[3];
    float w[3];
    sq_triangle_of(m, ci, cj, up, fa, fb, v, w, &t);
    t.qx = qx; t.qz = qz;
    // a caller that reads the one footprint only (SqMesh: everything in the query's own frame) may leave the tile record out
    if constexpr (std::is_invocable_v<Found&, const int*, const float*, const SqTile&>) found(v, w, t);
    else found(v, w);
}

// one query: out = (px, py, pz, nx, ny, nz, white, residual); on the tiling the residual is taken in the base tile's frame and the
// tile offset added to px and pz last
template <typename Mesh>
MW_HD void sq_query_point(const Mesh& m, int mode, float qx, float qz, int iters, float out[8]) {
    sq_locate(m, mode, qx, qz, iters, [&] { for (int k = 0; k < 8; k++) out[k] = NAN; }, [&](const int v[3], const float w[3], const SqTile& t) {
        const bool rest = mode == MW_SQ_REST;
        // the surface at the chosen rest point: gathered once
        float p[3] = {0.f, 0.f, 0.f}, n[3] = {0.f, 0.f, 0.f}, wh = 0.f;
        for (int k = 0; k < 3; k++) {
            const float x[3] = {sq_corner_x(m, t, v[k], k), m.vert[3 * v[k] + 1], sq_corner_z(m, t, v[k], k)};
            for (int c = 0; c < 3; c++) {
                p[c] += w[k] * x[c];
                n[c] += w[k] * m.norm[3 * v[k] + c];
            }
            wh += w[k] * m.white[(size_t)m.wstride * v[k]];
        }
        const float inv = 1.f / sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
        out[0] = p[0]; out[1] = p[1]; out[2] = p[2];
        if constexpr (Mesh::tiled) { out[0] = sq_shift(p[0], t.kx, m.period); out[2] = sq_shift(p[2], t.kz, m.period); }
        out[3] = n[0] * inv; out[4] = n[1] * inv; out[5] = n[2] * inv;
        out[6] = wh;
        out[7] = rest ? 0.f : sqrtf((p[0] - t.qx) * (p[0] - t.qx) + (p[2] - t.qz) * (p[2] - t.qz));
    });
}

// |displaced(u*).xz - (x, z)| of a located point, in the frame of t: the horizontal position accumulated as sq_query_point accumulates it
template <typename Mesh>
MW_HD float sq_residual(const Mesh& m, const int v[3], const float w[3], const SqTile& t) {
    float px = 0.f, pz = 0.f;
    for (int k = 0; k < 3; k++) {
        px += w[k] * sq_corner_x(m, t, v[k], k);
        pz += w[k] * sq_corner_z(m, t, v[k], k);
    }
    return sqrtf((px - t.qx) * (px - t.qx) + (pz - t.qz) * (pz - t.qz));
}

// one velocity query (mw_ocean_query_velocity): the point located exactly as sq_query_point locates it, the velocity of the water
// particle there -- the per-vertex velocities vel [R*R][3] interpolated with the weights of the position -- and the same residual.
// out = (vx, vy, vz, residual)
template <typename Mesh>
MW_HD void sq_velocity_point(const Mesh& m, const float* vel, int mode, float qx, float qz, int iters, float out[4]) {
    sq_locate(m, mode, qx, qz, iters, [&] { for (int k = 0; k < 4; k++) out[k] = NAN; }, [&](const int v[3], const float w[3], const SqTile& t) {
        float u[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < 3; k++)
            for (int c = 0; c < 3; c++) u[c] += w[k] * vel[3 * v[k] + c];
        out[0] = u[0]; out[1] = u[1]; out[2] = u[2];
        out[3] = mode == MW_SQ_REST ? 0.f : sq_residual(m, v, w, t);
    });
}

#if defined(__HIPCC__)
// One lane per query: a coalesced 8-byte load of the point, the walk's dependent 3-vertex gathers (L2 / Infinity Cache: the
// vertex array of a 1024^2 mesh is 12 MB), one final gather of positions, normals and whitecap, two 16-byte stores.
// Mesh: SqMesh, or SqTiled on a periodic handle (QuerySurface::launch).
template <typename Mesh>
__global__ __launch_bounds__(256) void k_query_surface(Mesh m, int mode, int iters, const float2* __restrict__ xz, int64_t n,
                                                       float4* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float2 q = xz[k];
    float r[8];
    sq_query_point(m, mode, q.x, q.y, iters, r);
    out[2 * k] = make_float4(r[0], r[1], r[2], r[3]);
    out[2 * k + 1] = make_float4(r[4], r[5], r[6], r[7]);
}
// One lane per query, as k_query_surface: the same walk, one final gather of the three corners' velocities, one 16-byte store.
template <typename Mesh>
__global__ __launch_bounds__(256) void k_query_velocity(Mesh m, const float* __restrict__ vel, int mode, int iters,
                                                        const float2* __restrict__ xz, int64_t n, float4* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float2 q = xz[k];
    float r[4];
    sq_velocity_point(m, vel, mode, q.x, q.y, iters, r);
    out[k] = make_float4(r[0], r[1], r[2], r[3]);
}
#endif

}  // namespace mw
