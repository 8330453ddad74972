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
// tile x, then tile z, then id (rct_better): a pure function of (frame, ray, reach).
//
// Hierarchy: raycast.h's implicit quadtree over the N x N cells of ONE tile, nb = (N-1)/B + 1 leaf blocks per side -- the tree of an
// (N+1) x (N+1) mesh whose last grid line is line 0 shifted by +P (rct_leaf_box gathers with that wrap), in the same layout, so
// rc_reduce_lds and k_rc_build_top serve it unchanged.  Instance k of the tree is every box shifted by sq_shift (monotone: the shifted
// box holds the shifted vertices) and re-padded by MW_RC_PAD of its shifted magnitude on x and z.
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
// and the kernels are instantiated in surface_tiled.hip, the translation unit compiled without contraction (sq_shift, sq_reduce and the
// column planes carry no strict scope of their own).
#pragma once
#include "raycast.h"

namespace mw {

#define MW_RCT_MAX_REACH 1024  // MW_RC_MAX_REACH of include/mistral_water.h (surface_services.inc checks the caller's reach against it)
#define MW_RCT_MAX_H 8     // cap of h: horizontal displacement beyond 7 periods is not followed
#define MW_RCT_WIDEN 4.f   // a column's interval grows by this many MW_RC_TSLACK of its ends
#define MW_RCT_STOP 8.f    // the stop rule's margin, in MW_RC_TSLACK of the next column's entry
#define MW_RCT_OUT_OF_REACH (-2)

// the tree of one tile of an N x N frame: the cells [0, N)^2, grid line N the wrapped line 0
MW_HD RcTree rct_tree(float* box, int N, int B) { return rc_tree(box, N + 1, B); }

// vertex on grid lines (i, j), 0 <= i, j <= N, of relative tile (kx, kz): its position into p, its index in the frame returned
MW_HD int rct_corner(const SqMesh& m, int i, int j, int kx, int kz, float p[3]) {
    const int N = m.R, wi = i == N ? 1 : 0, wj = j == N ? 1 : 0;
    const int v = (wi ? 0 : i) * N + (wj ? 0 : j);
    const float* q = m.vert + 3 * (size_t)v;
    p[0] = sq_shift(q[0], kx + wi, m.period);
    p[1] = q[1];
    p[2] = sq_shift(q[2], kz + wj, m.period);
    return v;
}
MW_HD RcV rct_vertex(const SqMesh& m, const RcRay& r, int i, int j, int kx, int kz) {
    float p[3];
    rct_corner(m, i, j, kx, kz, p);
    return rc_shear(r, p);
}

// the box of leaf (bx, bz) of tile 0: rc_leaf_box with the wrapped gather
MW_HD void rct_leaf_box(const SqMesh& m, const RcTree& t, int bx, int bz, float lo[3], float hi[3]) {
    MW_RC_STRICT
    for (int c = 0; c < 3; c++) { lo[c] = INFINITY; hi[c] = -INFINITY; }
    if (bx >= t.nb || bz >= t.nb) return;
    const int N = m.R;
    const int i0 = bx * t.B, i1 = i0 + t.B < N ? i0 + t.B : N;
    const int j0 = bz * t.B, j1 = j0 + t.B < N ? j0 + t.B : N;
    for (int i = i0; i <= i1; i++)
        for (int j = j0; j <= j1; j++) {
            float v[3];
            rct_corner(m, i, j, 0, 0, v);
            for (int c = 0; c < 3; c++) { lo[c] = fminf(lo[c], v[c]); hi[c] = fmaxf(hi[c], v[c]); }
        }
    for (int c = 0; c < 3; c++) {
        const float p = MW_RC_PAD * ((hi[c] - lo[c]) + fmaxf(fabsf(lo[c]), fabsf(hi[c])));
        lo[c] = lo[c] - p;
        hi[c] = hi[c] + p;
    }
}

// the whole tree, serially (the CPU shim; the device builds the same boxes with k_rct_build_leaves and k_rc_build_top)
MW_HD void rct_build_serial(const SqMesh& m, const RcTree& t) {
    const int S = 1 << t.D;
    for (int x = 0; x < S; x++)
        for (int z = 0; z < S; z++) {
            float lo[3], hi[3];
            rct_leaf_box(m, t, x, z, lo, hi);
            rc_store_box(t.box, rc_level_offset(t.D) + (int64_t)x * S + z, lo, hi);
        }
    for (int L = t.D - 1; L >= 0; L--) {
        const int s = 1 << L;
        for (int x = 0; x < s; x++)
            for (int z = 0; z < s; z++) {
                float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
                for (int a = 0; a < 2; a++)
                    for (int b = 0; b < 2; b++) {
                        float cl[3], ch[3];
                        rc_load_box(t.box, rc_level_offset(L + 1) + (int64_t)(2 * x + a) * (2 * s) + (2 * z + b), cl, ch);
                        rc_merge(lo, hi, cl, ch);
                    }
                rc_store_box(t.box, rc_level_offset(L) + (int64_t)x * s + z, lo, hi);
            }
    }
}

// ---- one ray ---------------------------------------------------------------------------------------------------------
// the best hit so far: t, the relative tile of the triangle's cell, the id.  Nothing yet: (+inf, INT32_MIN, INT32_MIN, -1), which no
// candidate with t = +inf betters.
struct RctBest {
    float t;
    int kx, kz, id;
};
MW_HD RctBest rct_none() {
    RctBest b;
    b.t = INFINITY;
    b.kx = b.kz = INT32_MIN;
    b.id = -1;
    return b;
}
MW_HD bool rct_better(float t, int kx, int kz, int id, const RctBest& b) {
    if (t != b.t) return t < b.t;
    if (kx != b.kx) return kx < b.kx;
    if (kz != b.kz) return kz < b.kz;
    return id < b.id;
}

// cells [i0, i1) x [j0, j1) of relative tile (kx, kz), both triangles of each: rc_cells with the wrapped gather and the tile in the order
MW_HD void rct_cells(const SqMesh& m, const RcRay& r, int i0, int i1, int j0, int j1, int kx, int kz, RctBest* best) {
    const int N = m.R;
    for (int i = i0; i < i1; i++) {
        RcV a = rct_vertex(m, r, i, j0, kx, kz), b = rct_vertex(m, r, i + 1, j0, kx, kz);
        for (int j = j0; j < j1; j++) {
            const RcV c = rct_vertex(m, r, i, j + 1, kx, kz), d = rct_vertex(m, r, i + 1, j + 1, kx, kz);
            const int id = 2 * (i * N + j);
            float t, U, V, W, det;
            // lower (i,j) (i+1,j) (i,j+1), then upper (i+1,j+1) (i+1,j) (i,j+1)
            if (rc_triangle(a, b, c, r.tmin, r.tmax, &t, &U, &V, &W, &det) && rct_better(t, kx, kz, id, *best)) {
                best->t = t; best->kx = kx; best->kz = kz; best->id = id;
            }
            if (rc_triangle(d, b, c, r.tmin, r.tmax, &t, &U, &V, &W, &det) && rct_better(t, kx, kz, id + 1, *best)) {
                best->t = t; best->kx = kx; best->kz = kz; best->id = id + 1;
            }
            a = c;
            b = d;
        }
    }
}

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

// Every instance that can reach into column (cx, cz): rc_trace's stackless walk with the instances (cx + u, cz + v), |u|, |v| <= h, as the
// children of one more level above the roots -- after an instance's root comes the next instance's -- each box that of its relative tile.
// rs is r with tmin raised to the column's entry, thi the column's exit: boxes are culled against [rs.tmin, min(thi, best t)], triangles
// accepted on r's own interval.  An instance outside the window is refused at its root.
MW_HD void rct_trace(const SqMesh& m, const RcTree& tr, const RcRay& r, const RcRay& rs, float thi, int cx, int cz, int h, int reach,
                     RctBest* best) {
    const int fx = r.dx < 0.f, fz = r.dz < 0.f;
    const bool xminor = fabsf(r.dx) >= fabsf(r.dz);
    const int N = m.R;
    int u = -h, v = -h, L = 0, x = 0, z = 0, off = 0;  // off = rc_level_offset(L): 4 off + 1 a level down
    for (;;) {
        const int kx = cx + u, kz = cz + v;
        const bool window = (kx >= -reach) & (kx <= reach) & (kz >= -reach) & (kz <= reach);
        float lo[3], hi[3];
        rc_load_box(tr.box, off + (x << L) + z, lo, hi);
        rct_shift_box(lo, hi, kx, kz, m.period);
        if (rc_slab(rs, lo, hi, fminf(best->t, thi)) & window) {
            if (L < tr.D) {
                L++;
                off = 4 * off + 1;
                x = 2 * x + fx;
                z = 2 * z + fz;
                continue;
            }
            const int i0 = x * tr.B, j0 = z * tr.B;  // a padding leaf's box is empty: i0, j0 < N here
            rct_cells(m, r, i0, i0 + tr.B < N ? i0 + tr.B : N, j0, j0 + tr.B < N ? j0 + tr.B : N, kx, kz, best);
        }
        for (;;) {
            if (L == 0) {  // the next instance
                if (++v > h) {
                    v = -h;
                    if (++u > h) return;
                }
                break;
            }
            const int ax = (x & 1) ^ fx, az = (z & 1) ^ fz;
            const int c = xminor ? (az << 1 | ax) : (ax << 1 | az);
            if (c < 3) {
                const int n = c + 1;
                const int nx = xminor ? (n & 1) : (n >> 1), nz = xminor ? (n >> 1) : (n & 1);
                x = (x & ~1) | (nx ^ fx);
                z = (z & ~1) | (nz ^ fz);
                break;
            }
            L--;
            off = (off - 1) >> 2;
            x >>= 1;
            z >>= 1;
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
MW_HD int rct_walk(const SqMesh& m, const RcTree& tr, const RcRay& r, int reach, RctBest* best) {
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
MW_HD void rct_finish(const SqMesh& m, const RcRay& r, bool valid, const RctBest& best, int status, int K0x, int K0z, float out[8],
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
    const int N = m.R, cell = best.id >> 1, i = cell / N, j = cell - i * N;
    const bool upper = (best.id & 1) != 0;
    // corners in sq_triangle order: lower (i,j) (i+1,j) (i,j+1), upper (i+1,j+1) (i+1,j) (i,j+1)
    float pa[3], pb[3], pc[3];
    int v[3];
    v[0] = rct_corner(m, upper ? i + 1 : i, upper ? j + 1 : j, best.kx, best.kz, pa);
    v[1] = rct_corner(m, i + 1, j, best.kx, best.kz, pb);
    v[2] = rct_corner(m, i, j + 1, best.kx, best.kz, pc);
    float t = best.t, U = 0.f, V = 0.f, W = 0.f, det = 1.f;
    rc_triangle(rc_shear(r, pa), rc_shear(r, pb), rc_shear(r, pc), r.tmin, r.tmax, &t, &U, &V, &W, &det);  // the search's own bits
    const float wa = U / det, wb = V / det, wc = W / det;
    out[0] = t;
    out[1] = sq_shift(r.ox + t * r.dx, K0x, m.period);
    out[2] = r.oy + t * r.dy;
    out[3] = sq_shift(r.oz + t * r.dz, K0z, m.period);
    float n[3];
    for (int c = 0; c < 3; c++) n[c] = (wa * m.norm[3 * v[0] + c] + wb * m.norm[3 * v[1] + c]) + wc * m.norm[3 * v[2] + c];
    const float inv = 1.f / sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    out[4] = n[0] * inv;
    out[5] = n[1] * inv;
    out[6] = n[2] * inv;
    out[7] = (wa * m.white[(size_t)m.wstride * v[0]] + wb * m.white[(size_t)m.wstride * v[1]]) + wc * m.white[(size_t)m.wstride * v[2]];
    // facing: rc_finish's, on the instance's float32 corners
    const float* q1 = upper ? pb : pc;
    const float* q2 = upper ? pc : pb;
    const double e1x = (double)q1[0] - (double)pa[0], e1y = (double)q1[1] - (double)pa[1], e1z = (double)q1[2] - (double)pa[2];
    const double e2x = (double)q2[0] - (double)pa[0], e2y = (double)q2[1] - (double)pa[1], e2z = (double)q2[2] - (double)pa[2];
    const double gx = e1y * e2z - e1z * e2y, gy = e1z * e2x - e1x * e2z, gz = e1x * e2y - e1y * e2x;
    const double dn = ((double)r.dx * gx + (double)r.dy * gy) + (double)r.dz * gz;
    hit[0] = best.id;
    hit[1] = dn < 0.0 ? 1 : -1;
    hit[2] = K0x + best.kx;
    hit[3] = K0z + best.kz;
}

// the ray reduced to the frame of its origin's tile; false for an invalid ray (rc_setup's rule, or an origin sq_reduce refuses)
MW_HD bool rct_setup(const SqMesh& m, const float ray[8], RcRay* r, int* K0x, int* K0z) {
    *K0x = *K0z = 0;
    if (!rc_setup(ray, r)) return false;
    float rx, rz;
    if (!sq_reduce(m.R, m.unit_width, m.period, r->ox, K0x, &rx) || !sq_reduce(m.R, m.unit_width, m.period, r->oz, K0z, &rz)) return false;
    const float reduced[8] = {rx, ray[1], rz, ray[3], ray[4], ray[5], ray[6], ray[7]};
    return rc_setup(reduced, r);
}
// one ray through the column walk
MW_HD void rct_cast(const SqMesh& m, const RcTree& tr, const float ray[8], int reach, float out[8], int hit[4]) {
    RcRay r;
    int K0x, K0z;
    const bool valid = rct_setup(m, ray, &r, &K0x, &K0z);
    RctBest best = rct_none();
    const int status = valid ? rct_walk(m, tr, r, reach, &best) : -1;
    rct_finish(m, r, valid, best, status, K0x, K0z, out, hit);
}
// one ray against every triangle of every window tile in (tile x, tile z, id) order: the tests' brute force.  No hit is always -1 here.
MW_HD void rct_cast_brute(const SqMesh& m, const float ray[8], int reach, float out[8], int hit[4]) {
    RcRay r;
    int K0x, K0z;
    const bool valid = rct_setup(m, ray, &r, &K0x, &K0z);
    RctBest best = rct_none();
    if (valid)
        for (int kx = -reach; kx <= reach; kx++)
            for (int kz = -reach; kz <= reach; kz++) rct_cells(m, r, 0, m.R, 0, m.R, kx, kz, &best);
    rct_finish(m, r, valid, best, -1, K0x, K0z, out, hit);
}

#if defined(__HIPCC__)
// k_rc_build_leaves over the cells of one tile: the same tiles of leaves, LDS reduction and layout, the leaf gather wrapped
__global__ __launch_bounds__(256) void k_rct_build_leaves(SqMesh m, RcTree tr) {
    __shared__ float4 s_lo[256], s_hi[256];
    const int T = tr.D >= 4 ? 16 : (1 << tr.D);
    const int tiles = (1 << tr.D) / T;
    const int tx = blockIdx.x / tiles, tz = blockIdx.x - tx * tiles;
    const int lt = threadIdx.x;
    if (lt < T * T) {
        const int lx = lt / T, lz = lt - lx * T;
        float lo[3], hi[3];
        rct_leaf_box(m, tr, tx * T + lx, tz * T + lz, lo, hi);
        rc_store_box(tr.box, rc_level_offset(tr.D) + ((int64_t)(tx * T + lx) << tr.D) + (tz * T + lz), lo, hi);
        s_lo[lt] = make_float4(lo[0], lo[1], lo[2], 0.f);
        s_hi[lt] = make_float4(hi[0], hi[1], hi[2], 0.f);
    }
    int L = tr.D;
    for (int s = T >> 1; s >= 1; s >>= 1) {
        L--;
        const int lx = lt / s, lz = lt - lx * s;
        float4 lo, hi;
        __syncthreads();
        if (lt < s * s) rc_reduce_lds(s_lo, s_hi, s, lx, lz, &lo, &hi);
        __syncthreads();
        if (lt < s * s) {
            s_lo[lt] = lo;
            s_hi[lt] = hi;
            float4* g = reinterpret_cast<float4*>(tr.box) + 2 * (rc_level_offset(L) + ((int64_t)(tx * s + lx) << L) + (tz * s + lz));
            g[0] = lo;
            g[1] = hi;
        }
    }
}
// One lane per ray: two 16-byte loads of the ray, the column walk, two 16-byte stores of the row and one of the hit.
__global__ __launch_bounds__(256) void k_raycast_tiled(SqMesh m, RcTree tr, const float4* __restrict__ rays, int64_t n, int reach,
                                                       float4* __restrict__ out, int4* __restrict__ hit) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float4 a = rays[2 * k], b = rays[2 * k + 1];
    const float ray[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
    float o[8];
    int h[4];
#if defined(__HIP_DEVICE_COMPILE__)
    // what only the last step reads waits in vector registers: the walk's nested loops need the scalar ones for their exec masks, and
    // with these ten held there too the allocator spills scalars into vector lanes
    asm volatile("" : "+v"(m.norm), "+v"(m.white), "+v"(m.wstride), "+v"(out), "+v"(hit), "+v"(reach));
#endif
    rct_cast(m, tr, ray, reach, o, h);
    out[2 * k] = make_float4(o[0], o[1], o[2], o[3]);
    out[2 * k + 1] = make_float4(o[4], o[5], o[6], o[7]);
    if (hit) hit[k] = make_int4(h[0], h[1], h[2], h[3]);
}
#endif

}  // namespace mw
