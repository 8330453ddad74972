// raycast.h -- first hit of many rays on the displaced ocean surface (mw_ocean_raycast, include/mistral_water.h).
//
// The surface is the triangle mesh mw_ocean_query_surface reads (surface_query.h): vertex (i, j) of the R x R grid at i*R + j, rest
// cell (i, j) holding the lower triangle (i,j) (i+1,j) (i,j+1) and the upper triangle (i+1,j+1) (i+1,j) (i,j+1), corners in the order of
// sq_triangle, triangle id 2*(i*(R-1) + j) + upper.
//
// Intersection: two-sided and watertight after Woop, Benthin and Wald (2013), every float32 operation strict (contract(off) scopes):
//   per ray      kz = axis of largest |d| (lowest index on ties), kx = (kz+1)%3, ky = (kx+1)%3, kx <-> ky when d[kz] < 0;
//                Sx = d[kx]/d[kz], Sy = d[ky]/d[kz], Sz = 1/d[kz];
//   per vertex   P' = P - o, (Px, Py, Pz) = (P'[kx] - Sx P'[kz], P'[ky] - Sy P'[kz], Sz P'[kz])   (rc_shear: a vertex has the same
//                sheared coordinates in every triangle that holds it);
//   per triangle U = Cx By - Cy Bx, V = Ax Cy - Ay Cx, W = Bx Ay - By Ax: each the edge function Qx Py - Qy Px of a directed edge P -> Q
//                (B->C, C->A, A->B), recomputed in float64 from the same float32 values when exactly 0 (rc_edge);
//                hit when U, V, W are all >= 0 or all <= 0 and det = (U+V)+W != 0; T = (U Az + V Bz) + W Cz, t = T / det,
//                accepted when tmin <= t <= tmax.  The weights of A, B, C are U/det, V/det, W/det.
// A shared edge enters its two triangles in the same or in the opposite direction, so its two edge values are bitwise equal or exact
// negatives, and the two-sided sign test leaves no crack between triangles.
//
// First hit: the smallest accepted t over all triangles, ties to the smallest id: a pure function of (mesh, ray), whatever the
// hierarchy, the traversal order or the batch.
//
// Hierarchy (built on every call): a leaf covers a B x B block of cells, its box the AABB of the block's (B+1)^2 vertices inflated by
// MW_RC_PAD of its size; leaves merge 2 x 2 into an implicit complete quadtree, level L a 2^L x 2^L grid of nodes stored level by
// level, row-major (x the row), from rc_level_offset(L); padding nodes hold empty boxes (lo = +inf, hi = -inf).  Build: k_rc_build_leaves
// (one workgroup per 16 x 16 leaves, reduced in LDS to the tile's root) and, for trees deeper than 4 levels, k_rc_build_top (one
// workgroup, the top levels in LDS).
//
// Traversal (k_raycast, one lane per ray): stackless over the implicit tree.  The children of a node are visited in a per-ray order
// (the near half along x and along z first, the axis of the larger |d| varying fastest); the next node is the next sibling in that order
// or, after the last, the parent's next sibling: index arithmetic, no per-lane arrays.  A node is entered when its slab interval,
// widened by MW_RC_TSLACK of its ends' magnitudes (>= 2 gamma_3, Ize 2013), meets [tmin, min(tmax, best t)]: a box whose entry
// distance equals the best t is still entered, so a tie with a smaller id is found.
//
// One footprint or one tile: the leaf box, the builds, the cell test, the sibling step and the hit row are templates on the mesh type, as
// the other surface services are.  SqMesh is the R x R footprint above; SqTiled is one tile of the tiling raycast_tiled.h casts on, its
// N x N cells the tree of an (N+1) x (N+1) mesh whose last grid line is line 0 a period on.  The two differ in rc_side (cells per side,
// which is also the stride of the ids), in rc_corner (how a grid vertex is fetched) and in the order rc_keep keeps (the tiling puts the
// tile between t and id); everything else is one body, so both fetch and shear a vertex the same way.
//
// Everything but the __global__ wrappers is MW_HD: tests/raycast_shim.cpp compiles the same functions with g++ -ffp-contract=off.  Every
// function here that does float arithmetic carries MW_RC_STRICT, but SqTiled's rc_corner calls sq_shift, which has no strict scope: the
// SqTiled instantiations belong to a translation unit compiled without contraction (surface_tiled.hip) and to the g++ shims.
#pragma once
#include "mw_math.h"
#include "surface_query.h"

namespace mw {

#if defined(__clang__)
#define MW_RC_STRICT _Pragma("clang fp contract(off)")
#else
#define MW_RC_STRICT
#endif

#define MW_RC_DEFAULT_BLOCK 2              // leaf block side B in cells: the fastest of tools/raycast_bench.py's sweep
#define MW_RC_MAX_LEVEL 9                  // deepest leaf level: k_rc_build_top holds level D - 4, at most 32 x 32 nodes, in LDS
#define MW_RC_PAD 6.103515625e-05f         // 2^-14: a leaf box grows on every side by this fraction of its extent plus its magnitude
#define MW_RC_TSLACK 9.5367431640625e-07f  // 2^-20 >= 2 gamma_3 = 6u / (1 - 3u), u = 2^-24

// the hierarchy: box [nodes][8] floats = lo.x lo.y lo.z 0 hi.x hi.y hi.z 0
struct RcTree {
    float* box;
    int B;   // leaf block side, cells
    int nb;  // leaf blocks per side
    int D;   // leaf level: 2^D >= nb
};

MW_HD int64_t rc_level_offset(int L) { return (((int64_t)1 << (2 * L)) - 1) / 3; }
MW_HD int64_t rc_nodes(int D) { return rc_level_offset(D + 1); }
// the geometry of the tree of an R x R mesh (R >= 2) with leaf blocks of B cells
MW_HD RcTree rc_tree(float* box, int R, int B) {
    RcTree t;
    t.box = box;
    t.B = B;
    t.nb = (R - 2) / B + 1;
    t.D = 0;
    while ((1 << t.D) < t.nb) t.D++;
    return t;
}

MW_HD float rc_sel3(float a, float b, float c, int k) { return k == 0 ? a : (k == 1 ? b : c); }
MW_HD bool rc_finite(float x) { return fabsf(x) <= 3.40282347e38f; }

// ---- what the mesh type decides ------------------------------------------------------------------------------------------
// cells per side, and so the stride of the triangle ids 2*(i*side + j) + upper
template <typename Mesh>
MW_HD int rc_side(const Mesh& m) { return Mesh::tiled ? m.R : m.R - 1; }
// vertex on grid lines (i, j), 0 <= i, j <= rc_side: its position into p, its index in the frame returned.  The footprint reads it where
// it lies and has no tiles; the tiling wraps line N to line 0 of the next tile and places relative tile (kx, kz) with sq_shift -- a vertex
// on grid line g = k N + a is always sq_shift(v[a], k, P), whichever cell or tile asks.
template <typename Mesh>
MW_HD int rc_corner(const Mesh& m, int i, int j, int kx, int kz, float p[3]) {
    if constexpr (Mesh::tiled) {
        const int N = m.R, wi = i == N ? 1 : 0, wj = j == N ? 1 : 0;
        const int v = (wi ? 0 : i) * N + (wj ? 0 : j);
        const float* q = m.vert + 3 * (size_t)v;
        p[0] = sq_shift(q[0], kx + wi, m.period);
        p[1] = q[1];
        p[2] = sq_shift(q[2], kz + wj, m.period);
        return v;
    } else {
        const int v = i * m.R + j;
        const float* q = m.vert + 3 * (size_t)v;
        p[0] = q[0]; p[1] = q[1]; p[2] = q[2];
        return v;
    }
}
// the best hit so far: t, the relative tile of the triangle's cell (the footprint leaves it alone), the id.  Nothing yet:
// (+inf, INT32_MIN, INT32_MIN, -1), which no candidate with t = +inf betters.
struct RcBest {
    float t;
    int kx, kz, id;
};
MW_HD RcBest rc_none() {
    RcBest b;
    b.t = INFINITY;
    b.kx = b.kz = INT32_MIN;
    b.id = -1;
    return b;
}
// keeps the candidate when it comes first: by (t, id) on the footprint, by (t, tile x, tile z, id) on the tiling
template <typename Mesh>
MW_HD void rc_keep(float t, int kx, int kz, int id, RcBest* b) {
    bool better;
    if constexpr (Mesh::tiled) better = t != b->t ? t < b->t : (kx != b->kx ? kx < b->kx : (kz != b->kz ? kz < b->kz : id < b->id));
    else better = t < b->t || (t == b->t && id < b->id);
    if (better) { b->t = t; b->kx = kx; b->kz = kz; b->id = id; }
}

// ---- the hierarchy ---------------------------------------------------------------------------------------------------
// the box of leaf (bx, bz): the AABB of its block's vertices (of tile 0), inflated; empty for padding leaves
template <typename Mesh>
MW_HD void rc_leaf_box(const Mesh& m, const RcTree& t, int bx, int bz, float lo[3], float hi[3]) {
    MW_RC_STRICT
    for (int c = 0; c < 3; c++) { lo[c] = INFINITY; hi[c] = -INFINITY; }
    if (bx >= t.nb || bz >= t.nb) return;
    const int S = rc_side(m);
    const int i0 = bx * t.B, i1 = i0 + t.B < S ? i0 + t.B : S;
    const int j0 = bz * t.B, j1 = j0 + t.B < S ? j0 + t.B : S;
    for (int i = i0; i <= i1; i++)
        for (int j = j0; j <= j1; j++) {
            float v[3];
            rc_corner(m, i, j, 0, 0, v);
            for (int c = 0; c < 3; c++) { lo[c] = fminf(lo[c], v[c]); hi[c] = fmaxf(hi[c], v[c]); }
        }
    for (int c = 0; c < 3; c++) {
        const float p = MW_RC_PAD * ((hi[c] - lo[c]) + fmaxf(fabsf(lo[c]), fabsf(hi[c])));
        lo[c] = lo[c] - p;
        hi[c] = hi[c] + p;
    }
}
MW_HD void rc_store_box(float* box, int64_t node, const float lo[3], const float hi[3]) {
    float* b = box + 8 * node;
    b[0] = lo[0]; b[1] = lo[1]; b[2] = lo[2]; b[3] = 0.f;
    b[4] = hi[0]; b[5] = hi[1]; b[6] = hi[2]; b[7] = 0.f;
}
MW_HD void rc_load_box(const float* box, int64_t node, float lo[3], float hi[3]) {
#if defined(__HIP_DEVICE_COMPILE__)
    const float4* b = reinterpret_cast<const float4*>(box) + 2 * node;
    const float4 l = b[0], h = b[1];
    lo[0] = l.x; lo[1] = l.y; lo[2] = l.z;
    hi[0] = h.x; hi[1] = h.y; hi[2] = h.z;
#else
    const float* b = box + 8 * node;
    lo[0] = b[0]; lo[1] = b[1]; lo[2] = b[2];
    hi[0] = b[4]; hi[1] = b[5]; hi[2] = b[6];
#endif
}
MW_HD void rc_merge(float lo[3], float hi[3], const float cl[3], const float ch[3]) {
    for (int c = 0; c < 3; c++) { lo[c] = fminf(lo[c], cl[c]); hi[c] = fmaxf(hi[c], ch[c]); }
}

// the whole tree, serially (the CPU shim; the device builds the same boxes with k_rc_build_leaves and k_rc_build_top)
template <typename Mesh>
MW_HD void rc_build_serial(const Mesh& m, const RcTree& t) {
    const int S = 1 << t.D;
    for (int x = 0; x < S; x++)
        for (int z = 0; z < S; z++) {
            float lo[3], hi[3];
            rc_leaf_box(m, t, x, z, lo, hi);
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
struct RcRay {
    float ox, oy, oz, dx, dy, dz, tmin, tmax;
    float ix, iy, iz;                 // 1 / d per axis (+-inf for a zero component)
    float okx, oky, okz, sx, sy, sz;  // o permuted to (kx, ky, kz); Sx, Sy, Sz
    int kx, ky, kz;
};
// false for an invalid ray: o or d not finite, d = 0, tmin < 0, tmin > tmax, either NaN
MW_HD bool rc_setup(const float in[8], RcRay* r) {
    MW_RC_STRICT
    r->ox = in[0]; r->oy = in[1]; r->oz = in[2]; r->tmin = in[3];
    r->dx = in[4]; r->dy = in[5]; r->dz = in[6]; r->tmax = in[7];
    if (!(rc_finite(r->ox) && rc_finite(r->oy) && rc_finite(r->oz) && rc_finite(r->dx) && rc_finite(r->dy) && rc_finite(r->dz)))
        return false;
    if (r->dx == 0.f && r->dy == 0.f && r->dz == 0.f) return false;
    if (!(r->tmin >= 0.f && r->tmin <= r->tmax)) return false;
    const float ax = fabsf(r->dx), ay = fabsf(r->dy), az = fabsf(r->dz);
    int kz = 0;
    if (ay > ax) kz = 1;
    if (az > rc_sel3(ax, ay, az, kz)) kz = 2;
    int kx = kz == 2 ? 0 : kz + 1;
    int ky = kx == 2 ? 0 : kx + 1;
    const float dkz = rc_sel3(r->dx, r->dy, r->dz, kz);
    if (dkz < 0.f) { const int s = kx; kx = ky; ky = s; }
    r->kx = kx; r->ky = ky; r->kz = kz;
    r->sx = rc_sel3(r->dx, r->dy, r->dz, kx) / dkz;
    r->sy = rc_sel3(r->dx, r->dy, r->dz, ky) / dkz;
    r->sz = 1.f / dkz;
    r->okx = rc_sel3(r->ox, r->oy, r->oz, kx);
    r->oky = rc_sel3(r->ox, r->oy, r->oz, ky);
    r->okz = rc_sel3(r->ox, r->oy, r->oz, kz);
    r->ix = 1.f / r->dx; r->iy = 1.f / r->dy; r->iz = 1.f / r->dz;
    return true;
}

// sheared coordinates of a vertex: (x, y) in the ray's projected plane, z = Sz (P - o)[kz]
struct RcV {
    float x, y, z;
};
MW_HD RcV rc_shear(const RcRay& r, const float* p) {
    MW_RC_STRICT
    const float px = p[0], py = p[1], pz = p[2];
    const float ax = rc_sel3(px, py, pz, r.kx) - r.okx;
    const float ay = rc_sel3(px, py, pz, r.ky) - r.oky;
    const float az = rc_sel3(px, py, pz, r.kz) - r.okz;
    RcV s;
    s.x = ax - r.sx * az;
    s.y = ay - r.sy * az;
    s.z = r.sz * az;
    return s;
}
// the edge function of the directed edge P -> Q: Qx Py - Qy Px, in float64 from the same values when it is exactly 0 in float32
MW_HD float rc_edge(const RcV& p, const RcV& q) {
    MW_RC_STRICT
    float e = q.x * p.y - q.y * p.x;
    if (e == 0.f) e = (float)((double)q.x * (double)p.y - (double)q.y * (double)p.x);
    return e;
}
// triangle A B C (sq_triangle order): true, t and U, V, W, det when the ray hits it inside [tmin, tmax]
MW_HD bool rc_triangle(const RcV& A, const RcV& B, const RcV& C, float tmin, float tmax, float* t, float* U, float* V, float* W,
                       float* det) {
    MW_RC_STRICT
    const float u = rc_edge(B, C), v = rc_edge(C, A), w = rc_edge(A, B);
    if ((u < 0.f || v < 0.f || w < 0.f) && (u > 0.f || v > 0.f || w > 0.f)) return false;
    const float d = (u + v) + w;
    if (d == 0.f) return false;
    const float tt = ((u * A.z + v * B.z) + w * C.z) / d;
    if (!(tt >= tmin && tt <= tmax)) return false;  // NaN (a non-finite vertex) is no hit
    *t = tt; *U = u; *V = v; *W = w; *det = d;
    return true;
}

// the sheared vertex on grid lines (i, j) of relative tile (kx, kz)
template <typename Mesh>
MW_HD RcV rc_vertex(const Mesh& m, const RcRay& r, int i, int j, int kx, int kz) {
    float p[3];
    rc_corner(m, i, j, kx, kz, p);
    return rc_shear(r, p);
}
// cells [i0, i1) x [j0, j1) of relative tile (kx, kz), both triangles of each, in id order: keeps the first hit in *best.  Along j a
// cell's corners (i,j+1) (i+1,j+1) are the next cell's (i,j) (i+1,j): sheared once (a vertex's sheared coordinates do not depend on the
// cell).
template <typename Mesh>
MW_HD void rc_cells(const Mesh& m, const RcRay& r, int i0, int i1, int j0, int j1, int kx, int kz, RcBest* best) {
    const int S = rc_side(m);
    for (int i = i0; i < i1; i++) {
        RcV a = rc_vertex(m, r, i, j0, kx, kz), b = rc_vertex(m, r, i + 1, j0, kx, kz);
        for (int j = j0; j < j1; j++) {
            const RcV c = rc_vertex(m, r, i, j + 1, kx, kz), d = rc_vertex(m, r, i + 1, j + 1, kx, kz);
            const int id = 2 * (i * S + j);
            float t, U, V, W, det;
            // lower (i,j) (i+1,j) (i,j+1), then upper (i+1,j+1) (i+1,j) (i,j+1)
            if (rc_triangle(a, b, c, r.tmin, r.tmax, &t, &U, &V, &W, &det)) rc_keep<Mesh>(t, kx, kz, id, best);
            if (rc_triangle(d, b, c, r.tmin, r.tmax, &t, &U, &V, &W, &det)) rc_keep<Mesh>(t, kx, kz, id + 1, best);
            a = c;
            b = d;
        }
    }
}

// slab test of a box against [tmin, tlimit], the interval widened by MW_RC_TSLACK of its ends' magnitudes.  The near and far planes
// of an axis follow the sign of 1/d (+-inf for a zero component); a NaN from 0 * inf (the origin on a plane the ray runs along) leaves
// the axis unconstrained, and an empty box gives t0 = +inf, t0 - inf = NaN: refused.
MW_HD bool rc_slab(const RcRay& r, const float lo[3], const float hi[3], float tlimit) {
    MW_RC_STRICT
    const float nx = ((r.ix < 0.f ? hi[0] : lo[0]) - r.ox) * r.ix, fx = ((r.ix < 0.f ? lo[0] : hi[0]) - r.ox) * r.ix;
    const float ny = ((r.iy < 0.f ? hi[1] : lo[1]) - r.oy) * r.iy, fy = ((r.iy < 0.f ? lo[1] : hi[1]) - r.oy) * r.iy;
    const float nz = ((r.iz < 0.f ? hi[2] : lo[2]) - r.oz) * r.iz, fz = ((r.iz < 0.f ? lo[2] : hi[2]) - r.oz) * r.iz;
    float t0 = fmaxf(fmaxf(fmaxf(-INFINITY, nx), ny), nz);
    float t1 = fminf(fminf(fminf(INFINITY, fx), fy), fz);
    t0 = t0 - fabsf(t0) * MW_RC_TSLACK;
    t1 = t1 + fabsf(t1) * MW_RC_TSLACK;
    return t0 <= t1 && t0 <= tlimit && t1 >= r.tmin;
}

// The place of a stackless walk in the implicit tree: node (x, z) of level L, off = rc_level_offset(L).  The children of a node are
// visited in the ray's order: fx, fz = 1 where the ray runs down the axis (child bit 1 is then the near half), xminor when x varies
// fastest.
struct RcCursor {
    int L, x, z, off;
    MW_HD int node() const { return off + (x << L) + z; }
    // to the first child in the ray's order
    MW_HD void descend(int fx, int fz) { L++; off = 4 * off + 1; x = 2 * x + fx; z = 2 * z + fz; }
    // to the next sibling in the ray's order, else the parent's next sibling; false, at the root, when there is none
    MW_HD bool next(int fx, int fz, bool xminor) {
        for (;;) {
            if (L == 0) return false;
            const int ax = (x & 1) ^ fx, az = (z & 1) ^ fz;
            const int c = xminor ? (az << 1 | ax) : (ax << 1 | az);
            if (c < 3) {
                const int n = c + 1;
                const int nx = xminor ? (n & 1) : (n >> 1), nz = xminor ? (n >> 1) : (n & 1);
                x = (x & ~1) | (nx ^ fx);
                z = (z & ~1) | (nz ^ fz);
                return true;
            }
            L--; off = (off - 1) >> 2; x >>= 1; z >>= 1;
        }
    }
};
// the cells of leaf (x, z): a padding leaf's box is empty, so x B, z B < rc_side here
template <typename Mesh>
MW_HD void rc_leaf_cells(const Mesh& m, const RcTree& tr, const RcRay& r, int x, int z, int kx, int kz, RcBest* best) {
    const int S = rc_side(m), i0 = x * tr.B, j0 = z * tr.B;
    rc_cells(m, r, i0, i0 + tr.B < S ? i0 + tr.B : S, j0, j0 + tr.B < S ? j0 + tr.B : S, kx, kz, best);
}

// first hit through the hierarchy: *best stays rc_none() when nothing is hit
MW_HD void rc_trace(const SqMesh& m, const RcTree& tr, const RcRay& r, RcBest* best) {
    const int fx = r.dx < 0.f, fz = r.dz < 0.f;
    const bool xminor = fabsf(r.dx) >= fabsf(r.dz);  // the axis of the larger |d| varies fastest
    RcCursor cur = {0, 0, 0, 0};
    for (;;) {
        float lo[3], hi[3];
        rc_load_box(tr.box, cur.node(), lo, hi);
        if (rc_slab(r, lo, hi, fminf(best->t, r.tmax))) {
            if (cur.L < tr.D) {
                cur.descend(fx, fz);
                continue;
            }
            rc_leaf_cells(m, tr, r, cur.x, cur.z, 0, 0, best);
        }
        if (!cur.next(fx, fz, xminor)) return;
    }
}

// The row of a hit but for where the surface stands: out[0] = t and out[4..7] = normal and whitecap, hit = (id, facing); the caller
// places out[1..3].  The corners of triangle best.id of relative tile (best.kx, best.kz) in sq_triangle order -- lower (i,j) (i+1,j)
// (i,j+1), upper (i+1,j+1) (i+1,j) (i,j+1) -- go through rc_triangle once more for the search's own bits.
template <typename Mesh>
MW_HD void rc_hit_row(const Mesh& m, const RcRay& r, const RcBest& best, float out[8], int hit[2]) {
    MW_RC_STRICT
    const int S = rc_side(m), cell = best.id >> 1, i = cell / S, j = cell - i * S;
    const bool upper = (best.id & 1) != 0;
    float pa[3], pb[3], pc[3];
    int v[3];
    v[0] = rc_corner(m, upper ? i + 1 : i, upper ? j + 1 : j, best.kx, best.kz, pa);
    v[1] = rc_corner(m, i + 1, j, best.kx, best.kz, pb);
    v[2] = rc_corner(m, i, j + 1, best.kx, best.kz, pc);
    float t = best.t, U = 0.f, V = 0.f, W = 0.f, det = 1.f;
    rc_triangle(rc_shear(r, pa), rc_shear(r, pb), rc_shear(r, pc), r.tmin, r.tmax, &t, &U, &V, &W, &det);
    const float wa = U / det, wb = V / det, wc = W / det;
    out[0] = t;
    float n[3];
    for (int c = 0; c < 3; c++) n[c] = (wa * m.norm[3 * v[0] + c] + wb * m.norm[3 * v[1] + c]) + wc * m.norm[3 * v[2] + c];
    const float inv = 1.f / sqrtf((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
    out[4] = n[0] * inv;
    out[5] = n[1] * inv;
    out[6] = n[2] * inv;
    out[7] = (wa * m.white[(size_t)m.wstride * v[0]] + wb * m.white[(size_t)m.wstride * v[1]]) + wc * m.white[(size_t)m.wstride * v[2]];
    // facing: the sign of d . n_g in float64, n_g = e1 x e2 the displaced triangle's normal oriented as the rest triangle's +y, on the
    // float32 corners (lower: e1 = C - A, e2 = B - A; upper: e1 = B - A, e2 = C - A)
    const float* q1 = upper ? pb : pc;
    const float* q2 = upper ? pc : pb;
    const double e1x = (double)q1[0] - (double)pa[0], e1y = (double)q1[1] - (double)pa[1], e1z = (double)q1[2] - (double)pa[2];
    const double e2x = (double)q2[0] - (double)pa[0], e2y = (double)q2[1] - (double)pa[1], e2z = (double)q2[2] - (double)pa[2];
    const double gx = e1y * e2z - e1z * e2y, gy = e1z * e2x - e1x * e2z, gz = e1x * e2y - e1y * e2x;
    const double dn = ((double)r.dx * gx + (double)r.dy * gy) + (double)r.dz * gz;
    hit[0] = best.id;
    hit[1] = dn < 0.0 ? 1 : -1;
}

// the row of a ray: out = t px py pz nx ny nz white, hit = (id, facing); misses and invalid rays as include/mistral_water.h says
MW_HD void rc_finish(const SqMesh& m, const RcRay& r, bool valid, const RcBest& best, float out[8], int hit[2]) {
    MW_RC_STRICT
    for (int k = 0; k < 8; k++) out[k] = NAN;
    hit[0] = -1;
    hit[1] = 0;
    if (!valid) return;
    if (best.id < 0) {
        out[0] = INFINITY;
        return;
    }
    rc_hit_row(m, r, best, out, hit);
    out[1] = r.ox + out[0] * r.dx;
    out[2] = r.oy + out[0] * r.dy;
    out[3] = r.oz + out[0] * r.dz;
}

// one ray through the hierarchy
MW_HD void rc_cast(const SqMesh& m, const RcTree& tr, const float ray[8], float out[8], int hit[2]) {
    RcRay r;
    const bool valid = rc_setup(ray, &r);
    RcBest best = rc_none();
    if (valid) rc_trace(m, tr, r, &best);
    rc_finish(m, r, valid, best, out, hit);
}
// one ray against every triangle in id order: the same intersection without a hierarchy (the tests' brute force)
MW_HD void rc_cast_brute(const SqMesh& m, const float ray[8], float out[8], int hit[2]) {
    RcRay r;
    const bool valid = rc_setup(ray, &r);
    RcBest best = rc_none();
    if (valid) rc_cells(m, r, 0, m.R - 1, 0, m.R - 1, 0, 0, &best);
    rc_finish(m, r, valid, best, out, hit);
}

#if defined(__HIPCC__)
// the 2 x 2 children of node (lx, lz) of an s x s level, held in LDS as the 2s x 2s level below it
__device__ __forceinline__ void rc_reduce_lds(const float4* s_lo, const float4* s_hi, int s, int lx, int lz, float4* lo, float4* hi) {
    *lo = make_float4(INFINITY, INFINITY, INFINITY, 0.f);
    *hi = make_float4(-INFINITY, -INFINITY, -INFINITY, 0.f);
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++) {
            const int q = (2 * lx + a) * (2 * s) + 2 * lz + b;
            const float4 cl = s_lo[q], ch = s_hi[q];
            lo->x = fminf(lo->x, cl.x); lo->y = fminf(lo->y, cl.y); lo->z = fminf(lo->z, cl.z);
            hi->x = fmaxf(hi->x, ch.x); hi->y = fmaxf(hi->y, ch.y); hi->z = fmaxf(hi->z, ch.z);
        }
}
// Leaves and the levels above them up to level D - 4: one workgroup per T x T tile of leaves (T = min(16, 2^D)), one lane per leaf
// gathering its (B+1)^2 vertices, then the tile reduced 2 x 2 in LDS up to its own root; every level is written out.
template <typename Mesh>
__global__ __launch_bounds__(256) void k_rc_build_leaves(Mesh m, RcTree tr) {
    __shared__ float4 s_lo[256], s_hi[256];
    const int T = tr.D >= 4 ? 16 : (1 << tr.D);
    const int tiles = (1 << tr.D) / T;
    const int tx = blockIdx.x / tiles, tz = blockIdx.x - tx * tiles;
    const int lt = threadIdx.x;
    if (lt < T * T) {
        const int lx = lt / T, lz = lt - lx * T;
        float lo[3], hi[3];
        rc_leaf_box(m, tr, tx * T + lx, tz * T + lz, lo, hi);
        rc_store_box(tr.box, rc_level_offset(tr.D) + ((int64_t)(tx * T + lx) << tr.D) + (tz * T + lz), lo, hi);
        s_lo[lt] = make_float4(lo[0], lo[1], lo[2], 0.f);
        s_hi[lt] = make_float4(hi[0], hi[1], hi[2], 0.f);
    }
    int L = tr.D;
    for (int s = T >> 1; s >= 1; s >>= 1) {  // level L - 1 of the tile: s x s nodes from the 2s x 2s below
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
// a ray's two 16-byte loads and its row's two 16-byte stores
__device__ __forceinline__ void rc_load_ray(const float4* __restrict__ rays, int64_t k, float ray[8]) {
    const float4 a = rays[2 * k], b = rays[2 * k + 1];
    ray[0] = a.x; ray[1] = a.y; ray[2] = a.z; ray[3] = a.w;
    ray[4] = b.x; ray[5] = b.y; ray[6] = b.z; ray[7] = b.w;
}
__device__ __forceinline__ void rc_store_row(float4* __restrict__ out, int64_t k, const float o[8]) {
    out[2 * k] = make_float4(o[0], o[1], o[2], o[3]);
    out[2 * k + 1] = make_float4(o[4], o[5], o[6], o[7]);
}
#if !defined(MW_RC_NO_KERNELS)  // the two kernels that are no templates are defined in one translation unit, mistral_water.hip
// The top levels of a tree deeper than 4: one workgroup reads level D - 4 (at most 32 x 32 nodes) into LDS and reduces it to the root.
__global__ __launch_bounds__(256) void k_rc_build_top(RcTree tr) {
    __shared__ float4 s_lo[1024], s_hi[1024];
    const int L0 = tr.D - 4, s0 = 1 << L0, lt = threadIdx.x;
    const float4* src = reinterpret_cast<const float4*>(tr.box) + 2 * rc_level_offset(L0);
    for (int k = lt; k < s0 * s0; k += 256) {
        s_lo[k] = src[2 * k];
        s_hi[k] = src[2 * k + 1];
    }
    for (int L = L0 - 1; L >= 0; L--) {  // level L: s x s nodes, s <= 16, one lane each
        const int s = 1 << L, lx = lt / s, lz = lt - lx * s;
        float4 lo, hi;
        __syncthreads();
        if (lt < s * s) rc_reduce_lds(s_lo, s_hi, s, lx, lz, &lo, &hi);
        __syncthreads();
        if (lt < s * s) {
            s_lo[lt] = lo;
            s_hi[lt] = hi;
            float4* g = reinterpret_cast<float4*>(tr.box) + 2 * (rc_level_offset(L) + lt);
            g[0] = lo;
            g[1] = hi;
        }
    }
}
// One lane per ray: the ray's loads, the stackless traversal (32 B per node, from L2), the leaves' vertex gathers, the row's stores and
// an 8-byte one of the hit.
__global__ __launch_bounds__(256) void k_raycast(SqMesh m, RcTree tr, const float4* __restrict__ rays, int64_t n, float4* __restrict__ out,
                                                 int2* __restrict__ hit) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    float ray[8], o[8];
    int h[2];
    rc_load_ray(rays, k, ray);
    rc_cast(m, tr, ray, o, h);
    rc_store_row(out, k, o);
    if (hit) hit[k] = make_int2(h[0], h[1]);
}
#endif  // MW_RC_NO_KERNELS
#endif

}  // namespace mw
