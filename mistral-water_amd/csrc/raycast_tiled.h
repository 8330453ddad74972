// raycast_tiled.h -- first hit of many rays on the tiled ocean surface (mw_ocean_raycast_tiled, include/mistral_water.h).
//
// The surface is the infinite tiling of an FFTMesh frame that surface_query.h defines (SqTiled): vertex (gi, gj) of the integer grid is
// vertex (ai, aj) of the frame displaced by (ki P, 0, kj P) through sq_shift, every integer cell exists -- the seam cells a = N-1, between
// the frame's last grid line and the next tile's first, included -- and each is split along the diagonal of raycast.h.  Tile (kx, kz)
// owns the N x N cells whose lower grid lines are its own; triangle id = 2 (ai N + aj) + upper.  The intersection is raycast.h's own
// (rc_setup, rc_shear, rc_edge, rc_triangle): a vertex on grid line g = k N + a is always sq_shift(v[a], k, P), whichever cell or tile
// asks, so its sheared coordinates are the same bits from both sides of a seam and the edge-function argument of raycast.h holds there.
//
// Reduction: K0 = the tile of the origin (sq_reduce on ox and oz), the ray is cast from o' = the reduced origin, in the frame of K0, where
// relative tile k has its vertices at sq_shift(v, k, P); K0 P is added to px and pz once, at the end.  The ray sees the (2 reach + 1)^2
// tiles within `reach` of K0.  First hit: the smallest accepted t over every triangle of every window tile, ties to the smallest relative
// tile x, then tile z, then id (rc_keep): a pure function of (frame, ray, reach).
//
// What is raycast.h's own, instantiated for SqTiled: the vertex fetch (rc_corner, which wraps grid line N to line 0 a period on), the leaf
// box and both builds, the cell test (rc_cells), the sibling step (RcCursor) and the hit row (rc_hit_row).  What is here belongs to the
// tiling alone: the instances and their shifted boxes, the window, the column walk, the reduction of the origin.
//
// Hierarchy: raycast.h's implicit quadtree over the N x N cells of ONE tile, nb = (N-1)/B + 1 leaf blocks per side -- the tree of an
// (N+1) x (N+1) mesh (rct_tree), built by rc_build_serial<SqTiled> / k_rc_build_leaves<SqTiled> and k_rc_build_top.  Instance k of the tree
// is every box shifted by sq_shift (monotone: the shifted box holds the shifted vertices) and re-padded by MW_RC_PAD of its shifted
// magnitude on x and z.
//
// Traversal (rct_walk, one lane per ray, no per-lane arrays):
//   1. [tmin, tmax] is clipped to the root box's height range, widened by MW_RC_TSLACK: [t0, t1].  Empty: a miss.
//   2. The columns of period P in the xz plane are walked in ray order; column c covers [sq_shift(x0, c, P), sq_shift(x0, c+1, P)] on
//      each axis, x0 = rest_coord(0).  Its t interval comes from those two planes per moving axis, widened by MW_RCT_WIDEN slacks of its
//      ends.  The exit plane of a column and the entry plane of the next are one expression -- the same bits -- so the unwidened intervals
//      abut and the widened ones overlap: no t of [t0, t1] falls between two columns.  The walk starts one column behind the column of
//      o' + t0 d on each moving axis, so a start misjudged by rounding is walked over, not skipped, and steps to the neighbour whose
//      exit is earlier.
//   3. In each column whose interval meets [t0, t1] the instances (c + u, c + v), |u|, |v| <= h, that lie in the window are traversed
//      (rct_trace: rc_trace's stackless walk over the shifted boxes), boxes culled against the column's interval cut to
//      [t0, min(t1, best t)], triangles accepted on the ray's own [tmin, tmax]: every candidate is a real hit of a real window triangle,
//      and the full (t, tile, id) comparison makes the order of columns and instances immaterial.  h = 1 + floor(overhang / P + 0.01),
//      the overhang how far the root box reaches beyond the footprint [x0, x0 + P]: a point of column c can only belong to a tile
//      within h of c, and the 0.01 P left over is orders of magnitude above the position error of a t at a column boundary.
//   4. The walk ends when the best t lies strictly below the next column's entry less MW_RCT_STOP slacks (a tie there is still found),
//      when [t0, t1] ends in this column, or when it steps past column reach + h -- beyond which no window tile reaches.  The last
//      case without a hit is "out of reach" (id -2).
//
// Everything but the __global__ wrappers is MW_HD: tests/raycast_tiled_shim.cpp compiles the same functions with g++ -ffp-contract=off,
// and k_raycast_tiled and k_rc_build_leaves<SqTiled> are instantiated in surface_tiled.hip, the translation unit compiled without
// contraction (sq_shift, sq_reduce and the column planes carry no strict scope of their own).
#pragma once
#include "raycast.h"

namespace mw {

#define MW_RCT_MAX_REACH 1024  // MW_RC_MAX_REACH of include/mistral_water.h: surface_tiled.hip, which sees both, asserts them equal
#define MW_RCT_MAX_H 8     // cap of h: horizontal displacement beyond 7 periods is not followed
#define MW_RCT_WIDEN 4.f   // a column's interval grows by this many MW_RC_TSLACK of its ends
#define MW_RCT_STOP 8.f    // the stop rule's margin, in MW_RC_TSLACK of the next column's entry
#define MW_RCT_OUT_OF_REACH (-2)

// the tree of one tile of an N x N frame: the cells [0, N)^2, grid line N the wrapped line 0
MW_HD RcTree rct_tree(float* box, int N, int B) { return rc_tree(box, N + 1, B); }
// The entry points (rct_build_serial, rct_cast, rct_cast_brute, k_raycast_tiled) take the frame as the SqMesh their callers hold, its
// period set, and read it as SqTiled from there on.  The whole tree of one tile, serially (the CPU shim):
MW_HD void rct_build_serial(const SqMesh& frame, const RcTree& t) { rc_build_serial(SqTiled{frame}, t); }

// a box of tile 0 as the box of relative tile (kx, kz): shifted, then padded by MW_RC_PAD of the magnitude it now has (the error of a
// slab distance scales with the coordinates it is computed from).  An empty box turns into NaN on x and z and stays empty on y: refused.
MW_HD void rct_shift_box(float lo[3], float hi[3], int kx, int kz, float P) {
    MW_RC_STRICT
    lo[0] = sq_shift(lo[0], kx, P); hi[0] = sq_shift(hi[0], kx, P);
    lo[2] = sq_shift(lo[2], kz, P); hi[2] = sq_shift(hi[2], kz, P);
    const float px = MW_RC_PAD * fmaxf(fabsf(lo[0]), fabsf(hi[0])), pz = MW_RC_PAD * fmaxf(fabsf(lo[2]), fabsf(hi[2]));
    lo[0] = lo[0] - px; hi[0] = hi[0] + px;
    lo[2] = lo[2] - pz; hi[2] = hi[2] + pz;
}

// Every instance that can reach into column (cx, cz): rc_trace's stackless walk (RcCursor) with the instances (cx + u, cz + v),
// |u|, |v| <= h, as the children of one more level above the roots -- after an instance's root comes the next instance's -- each box
// that of its relative tile.
// rs is r with tmin raised to the column's entry, thi the column's exit: boxes are culled against [rs.tmin, min(thi, best t)], triangles
// accepted on r's own interval.  An instance outside the window is refused at its root.
MW_HD void rct_trace(const SqTiled& m, const RcTree& tr, const RcRay& r, const RcRay& rs, float thi, int cx, int cz, int h, int reach,
                     RcBest* best) {
    const int fx = r.dx < 0.f, fz = r.dz < 0.f;
    const bool xminor = fabsf(r.dx) >= fabsf(r.dz);
    int u = -h, v = -h;
    RcCursor cur = {0, 0, 0, 0};
    for (;;) {
        const int kx = cx + u, kz = cz + v;
        const bool window = (kx >= -reach) & (kx <= reach) & (kz >= -reach) & (kz <= reach);
        float lo[3], hi[3];
        rc_load_box(tr.box, cur.node(), lo, hi);
        rct_shift_box(lo, hi, kx, kz, m.period);
        if (rc_slab(rs, lo, hi, fminf(best->t, thi)) & window) {
            if (cur.L < tr.D) {
                cur.descend(fx, fz);
                continue;
            }
            rc_leaf_cells(m, tr, r, cur.x, cur.z, kx, kz, best);
        }
        if (!cur.next(fx, fz, xminor) && ++v > h) {  // after an instance's root, the next instance
            v = -h;
            if (++u > h) return;
        }
    }
}

// how many tiles beyond its own column a tile's geometry can reach: 1 + floor(overhang / P + 0.01), from the root box
MW_HD int rct_overhang_tiles(const float lo[3], const float hi[3], float x0, float P) {
    MW_RC_STRICT
    const float x1 = sq_shift(x0, 1, P);
    const float over = fmaxf(fmaxf(x0 - lo[0], hi[0] - x1), fmaxf(x0 - lo[2], hi[2] - x1));
    const float q = over / P + 0.01f;
    if (!(q >= 1.f)) return 1;  // NaN too
    return q < (float)MW_RCT_MAX_H ? 1 + (int)floorf(q) : MW_RCT_MAX_H;
}
// the column of coordinate x, kept where an int holds it and the walk's bound still refuses it
MW_HD int rct_column(float x, float x0, float P) {
    MW_RC_STRICT
    return (int)fminf(fmaxf(floorf((x - x0) / P), -4.f * MW_RCT_MAX_REACH), 4.f * MW_RCT_MAX_REACH);
}

// the column walk: r is the ray in the frame of its origin's tile.  -1, or MW_RCT_OUT_OF_REACH when the walk left the columns the
// window's tiles reach; either way *best holds the first hit if there is one.
MW_HD int rct_walk(const SqTiled& m, const RcTree& tr, const RcRay& r, int reach, RcBest* best) {
    MW_RC_STRICT
    const float P = m.period, x0 = rest_coord(m.R, m.unit_width, 0);
    float lo[3], hi[3];
    rc_load_box(tr.box, 0, lo, hi);
    // 1. the height range of the surface
    float a = fmaxf(-INFINITY, ((r.iy < 0.f ? hi[1] : lo[1]) - r.oy) * r.iy);
    float c = fminf(INFINITY, ((r.iy < 0.f ? lo[1] : hi[1]) - r.oy) * r.iy);
    a = a - fabsf(a) * MW_RC_TSLACK;
    c = c + fabsf(c) * MW_RC_TSLACK;
    if (!(a <= c)) return -1;  // NaN: a level ray above or below the range
    const float t0 = fmaxf(r.tmin, a), t1 = fminf(r.tmax, c);
    if (!(t0 <= t1)) return -1;
    const int h = rct_overhang_tiles(lo, hi, x0, P), lim = reach + h;
    // 2. an axis moves when 1/d is finite; the start column, one behind on each moving axis
    const int sx = !rc_finite(r.ix) ? 0 : (r.dx > 0.f ? 1 : -1), sz = !rc_finite(r.iz) ? 0 : (r.dz > 0.f ? 1 : -1);
    int cx = rct_column(r.ox + t0 * r.dx, x0, P) - sx, cz = rct_column(r.oz + t0 * r.dz, x0, P) - sz;
    RcRay rs = r;
    for (;;) {
        if (cx > lim || cx < -lim || cz > lim || cz < -lim) return MW_RCT_OUT_OF_REACH;
        const float enx = sx == 0 ? -INFINITY : (sq_shift(x0, cx + (sx < 0 ? 1 : 0), P) - r.ox) * r.ix;
        const float exx = sx == 0 ? INFINITY : (sq_shift(x0, cx + (sx > 0 ? 1 : 0), P) - r.ox) * r.ix;
        const float enz = sz == 0 ? -INFINITY : (sq_shift(x0, cz + (sz < 0 ? 1 : 0), P) - r.oz) * r.iz;
        const float exz = sz == 0 ? INFINITY : (sq_shift(x0, cz + (sz > 0 ? 1 : 0), P) - r.oz) * r.iz;
        const float en = fmaxf(enx, enz), ex = fminf(exx, exz);
        const float cl = fmaxf(en - fabsf(en) * (MW_RCT_WIDEN * MW_RC_TSLACK), t0);
        const float ch = fminf(ex + fabsf(ex) * (MW_RCT_WIDEN * MW_RC_TSLACK), t1);
        if (cl <= ch) {  // 3. the instances that can reach into this column
            rs.tmin = cl;
            rct_trace(m, tr, r, rs, ch, cx, cz, h, reach, best);
        }
        // 4. the ray ends in this column, or nothing further on can come first
        if (ex >= t1) return -1;
        if (best->t < ex - fabsf(ex) * (MW_RCT_STOP * MW_RC_TSLACK)) return -1;
        if (sz == 0 || (sx != 0 && exx <= exz)) cx += sx;
        else cz += sz;
    }
}

// the row of a ray: out = t px py pz nx ny nz white, hit = (id, facing, tile x, tile z) as include/mistral_water.h says.  r is the ray
// in the frame of tile (K0x, K0z); status is rct_walk's.
MW_HD void rct_finish(const SqTiled& m, const RcRay& r, bool valid, const RcBest& best, int status, int K0x, int K0z, float out[8],
                      int hit[4]) {
    MW_RC_STRICT
    for (int k = 0; k < 8; k++) out[k] = NAN;
    hit[0] = -1;
    hit[1] = hit[2] = hit[3] = 0;
    if (!valid) return;
    if (best.id < 0) {
        out[0] = INFINITY;
        hit[0] = status;
        return;
    }
    rc_hit_row(m, r, best, out, hit);
    out[1] = sq_shift(r.ox + out[0] * r.dx, K0x, m.period);
    out[2] = r.oy + out[0] * r.dy;
    out[3] = sq_shift(r.oz + out[0] * r.dz, K0z, m.period);
    hit[2] = K0x + best.kx;
    hit[3] = K0z + best.kz;
}

// the ray reduced to the frame of its origin's tile; false for an invalid ray (rc_setup's rule, or an origin sq_reduce refuses)
MW_HD bool rct_setup(const SqTiled& m, const float ray[8], RcRay* r, int* K0x, int* K0z) {
    *K0x = *K0z = 0;
    if (!rc_setup(ray, r)) return false;
    float rx, rz;
    if (!sq_reduce(m.R, m.unit_width, m.period, r->ox, K0x, &rx) || !sq_reduce(m.R, m.unit_width, m.period, r->oz, K0z, &rz)) return false;
    const float reduced[8] = {rx, ray[1], rz, ray[3], ray[4], ray[5], ray[6], ray[7]};
    return rc_setup(reduced, r);
}
// one ray through the column walk
MW_HD void rct_cast(const SqMesh& frame, const RcTree& tr, const float ray[8], int reach, float out[8], int hit[4]) {
    const SqTiled m{frame};
    RcRay r;
    int K0x, K0z;
    const bool valid = rct_setup(m, ray, &r, &K0x, &K0z);
    RcBest best = rc_none();
    const int status = valid ? rct_walk(m, tr, r, reach, &best) : -1;
    rct_finish(m, r, valid, best, status, K0x, K0z, out, hit);
}
// one ray against every triangle of every window tile in (tile x, tile z, id) order: the tests' brute force.  No hit is always -1 here.
MW_HD void rct_cast_brute(const SqMesh& frame, const float ray[8], int reach, float out[8], int hit[4]) {
    const SqTiled m{frame};
    RcRay r;
    int K0x, K0z;
    const bool valid = rct_setup(m, ray, &r, &K0x, &K0z);
    RcBest best = rc_none();
    if (valid)
        for (int kx = -reach; kx <= reach; kx++)
            for (int kz = -reach; kz <= reach; kz++) rc_cells(m, r, 0, m.R, 0, m.R, kx, kz, &best);
    rct_finish(m, r, valid, best, -1, K0x, K0z, out, hit);
}

#if defined(__HIPCC__)
// One lane per ray: the ray's loads, the column walk, the row's stores and a 16-byte one of the hit.
__global__ __launch_bounds__(256) void k_raycast_tiled(SqMesh m, RcTree tr, const float4* __restrict__ rays, int64_t n, int reach,
                                                       float4* __restrict__ out, int4* __restrict__ hit) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    float ray[8], o[8];
    int h[4];
    rc_load_ray(rays, k, ray);
#if defined(__HIP_DEVICE_COMPILE__)
    // what only the last step reads waits in vector registers: the walk's nested loops need the scalar ones for their exec masks, and
    // with these ten held there too the allocator spills scalars into vector lanes
    asm volatile("" : "+v"(m.norm), "+v"(m.white), "+v"(m.wstride), "+v"(out), "+v"(hit), "+v"(reach));
#endif
    rct_cast(m, tr, ray, reach, o, h);
    rc_store_row(out, k, o);
    if (hit) hit[k] = make_int4(h[0], h[1], h[2], h[3]);
}
#endif

}  // namespace mw
