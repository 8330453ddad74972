// fleet.h -- mixed fleets: hull forces and floating bodies for many hull shapes in one call (mw_ocean_fleet_forces, mw_ocean_step_fleet,
// include/mistral_water.h).
//
// Up to MW_FLEET_HULLS hulls, their geometry concatenated (hull_xyz [total_verts][3], triangles [total_tris][3] with indices local to
// their hull), each with its own coefficients and its own count of bodies; the per-body arrays hold the bodies hull after hull.  A
// body's row and state are those of the single-hull kernels (hull_forces.h, rigid_bodies.h) on its hull alone, bit for bit: every
// kernel here reads (nverts, ntris, nchunks, coefficients, array offsets) per work item from the hull table and then calls what its
// single-hull counterpart calls: hull_vertex, hull_triangle, hull_chunk_partial, hull_body_sum, hull_row, body_integrate.  The order
// of a row's sum is hull_forces.h's alone; k_fleet_step repeats only k_bodies_step's phases around those calls.
//
// k_fleet_step is also the one-launch kernel of every strict single-hull call: mw_ocean_step_bodies on a periodic handle and
// mw_ocean_step_moored's one-launch plan run it on a one-hull table (surface_services.inc: hull_step_launch), the second with the
// body's mooring lines (moorings.h).  The substep loop therefore stands in two places, here and in k_bodies_step, which is the one
// kernel that cannot share it (rigid_bodies.h).
//
// The table travels by value in the kernel arguments (FleetTable, under 2 KiB): nothing to upload, so a second call enqueued before
// the first has run reads its own table.  A work index (instance vertex, (body, chunk) or body) maps to (hull, body, item) through
// the per-hull starts of that space: fleet_map, a loop over the hulls with a uniform index and compare-and-select, so that a lane-varying
// work index never indexes the table (which would copy it to scratch).
//
//   k_fleet_vertices   one lane per instance vertex over all hulls               (k_hull_vertices)
//   k_fleet_triangles  one 256-lane workgroup per (body, chunk) over all hulls   (k_hull_triangles)
//   k_fleet_reduce     one wave per body                                         (k_hull_reduce)
//   k_fleet_integrate  one lane per body, with the wrench                        (k_bodies_integrate)
//   k_fleet_step       one 256-lane workgroup per body runs every substep        (k_bodies_step; SqTiled only, see below), with
//                      the external wrench and the mooring lines, each optional
//
// Operand order.  The SqTiled instantiations are compiled without contraction (surface_tiled.hip), where equal operations give equal
// bits.  The SqMesh instantiations are compiled with contraction, and there the compiler fuses the FIRST product of a sum of two
// products, a * b + c * d -> fma(a, b, c * d), after an earlier pass has put the two products in an order of its own: the one defined
// from values that appear earlier in the kernel comes first.  hull_transform's R[3c] * h[0] + R[3c+1] * h[1] came out as
// fma(R[3c], h[0], R[3c+1] * h[1]) in a kernel that loads the pose before the hull vertex with the table's values read in between, and
// as fma(R[3c+1], h[1], R[3c] * h[0]) in k_hull_vertices: rows differed in the last bits.  So the kernels here load in the order that
// reproduces the single-hull kernels' operand order (checked on the optimised IR: the same sums of products, the same operand first).
// For two kernels no order of loads reproduced the single-hull sums (hull_transform's, and body_integrate's R^T tau and R dw):
// k_fleet_step is instantiated for SqTiled only, and on the one footprint a call without a wrench integrates with k_bodies_integrate
// itself, launched per hull (surface_services.inc: fleet_launch).  There every hull steps through the per-substep kernels, whose bits
// are those of both of mw_ocean_step_bodies' plans; k_fleet_integrate<SqMesh> runs only with a wrench, where no single-hull call
// defines the bits.
//
// Everything but the __global__ wrappers is MW_HD: tests/fleet_shim.cpp compiles the same functions with g++.
#pragma once
#include "moorings.h"  // the lines of k_fleet_step; rigid_bodies.h: the pushed row

namespace mw {

#define MW_FLEET_HULLS 32  // MW_FLEET_MAX_HULLS of the ABI

// the three work spaces of a table
#define MW_FLEET_VERTS 0   // nbodies * nverts:  one item per instance vertex
#define MW_FLEET_CHUNKS 1  // nbodies * nchunks: one item per (body, chunk)
#define MW_FLEET_BODIES 2  // nbodies

// one hull as the kernels read it
struct FleetHull {
    int vert_first, nverts, tri_first, ntris;  // its ranges of hull_xyz and triangles
    int nchunks;                               // ceil(max(ntris, nverts) / MW_HULL_CHUNK)
    int body_first;                            // its first body in the call's per-body arrays (bodies, mass, wrench, out, rows)
    int first[3];                              // where its work starts in each space of this table
    HullCoeffs cf;
    float vscale, g;
};
// The hulls of one group of launches.  Every hull of the call has its row; a hull that is not in the group (or has no bodies) has no
// work: first[s] of the next hull equals its own.
struct FleetTable {
    int nhulls;
    int total[3];  // the size of each space
    FleetHull hull[MW_FLEET_HULLS];
};

// the chunks of one hull of a table: a fleet's hull is chunked as a single hull is
MW_HD int fleet_chunks(int nverts, int ntris) { return hull_chunks(nverts, ntris); }

// Fills the geometry, body_first, first[] and total[] of t from a hull table hulls [nhulls][5] = vert_first, nverts, tri_first, ntris,
// nbodies (validated by the caller: nhulls in [1, MW_FLEET_HULLS], every sum below 2^31); hull h has work in t only when bit h of
// `take` is set.  The coefficients are the caller's to fill.
MW_HD void fleet_table(const int32_t* hulls, int nhulls, uint32_t take, FleetTable* t) {
    t->nhulls = nhulls;
    int body = 0, first[3] = {0, 0, 0};
    for (int h = 0; h < nhulls; h++) {
        const int32_t* r = hulls + 5 * h;
        FleetHull& f = t->hull[h];
        f.vert_first = r[0]; f.nverts = r[1]; f.tri_first = r[2]; f.ntris = r[3];
        f.nchunks = fleet_chunks(r[1], r[3]);
        f.body_first = body;
        for (int s = 0; s < 3; s++) f.first[s] = first[s];
        const int nb = ((take >> h) & 1u) ? r[4] : 0;
        first[MW_FLEET_VERTS] += nb * f.nverts;
        first[MW_FLEET_CHUNKS] += nb * f.nchunks;
        first[MW_FLEET_BODIES] += nb;
        body += r[4];
    }
    for (int s = 0; s < 3; s++) t->total[s] = first[s];
}

// Work item w of a space (0 <= w < t.total[space]): its hull, the body within that hull, the item within that body (vertex, chunk, 0)
// and the hull's row.  The starts are non-decreasing and a hull without work shares its start with the next one, so the last hull
// whose start is <= w is the one that holds w.  The table is only ever indexed by h, which is uniform.
struct FleetItem {
    int hull, body, item;
    FleetHull row;
};
static_assert(sizeof(FleetHull) == 15 * 4, "fleet_map selects FleetHull field by field: a new field needs its line there");
MW_HD FleetItem fleet_map(const FleetTable& t, int space, int w) {
    FleetItem it;
    it.hull = 0;
    it.row = t.hull[0];
    for (int h = 1; h < t.nhulls; h++) {
        const FleetHull r = t.hull[h];
        const bool in = w >= r.first[space];
        it.hull = in ? h : it.hull;
        // field by field: a select of the whole struct goes through memory (136 B of scratch in every kernel)
        it.row.vert_first = in ? r.vert_first : it.row.vert_first; it.row.nverts = in ? r.nverts : it.row.nverts;
        it.row.tri_first = in ? r.tri_first : it.row.tri_first;    it.row.ntris = in ? r.ntris : it.row.ntris;
        it.row.nchunks = in ? r.nchunks : it.row.nchunks;          it.row.body_first = in ? r.body_first : it.row.body_first;
        for (int s = 0; s < 3; s++) it.row.first[s] = in ? r.first[s] : it.row.first[s];
        it.row.cf.rho_g = in ? r.cf.rho_g : it.row.cf.rho_g; it.row.cf.lin = in ? r.cf.lin : it.row.cf.lin;
        it.row.cf.quad = in ? r.cf.quad : it.row.cf.quad;    it.row.cf.drag = in ? r.cf.drag : it.row.cf.drag;
        it.row.vscale = in ? r.vscale : it.row.vscale;       it.row.g = in ? r.g : it.row.g;
    }
    const unsigned per = space == MW_FLEET_VERTS ? (unsigned)it.row.nverts : space == MW_FLEET_CHUNKS ? (unsigned)it.row.nchunks : 1u;
    const unsigned local = (unsigned)(w - it.row.first[space]);
    it.body = (int)(local / per);
    it.item = (int)(local - (unsigned)it.body * per);
    return it;
}

#if defined(__HIPCC__)
template <typename Mesh>
struct FleetArgsT {
    Mesh m;
    const float* vel;  // per-vertex water velocity [R*R][3] (some hull has drag), else nullptr
    int iters;
    const float* hull;      // [total_verts][3]
    const int* tris;        // [total_tris][3], indices local to their hull
    float4* bodies;         // [total_bodies][4] float4; updated in place by the stepping kernels
    const float4* mass;     // [total_bodies][2]
    const float4* wrench;   // [total_bodies][2] or nullptr
    float4* vslab;          // [total[VERTS]][2]
    float4* part;           // [total[CHUNKS]][2]
    float4* rows;           // [total_bodies][2]: k_fleet_reduce writes them, k_fleet_integrate reads them
    float4* out;            // [total_bodies][2] or nullptr (stepping): the row of the last substep
    float dt;               // h = dt / substeps
    int substeps;
    int last;               // k_fleet_integrate: this is the call's last substep (write out)
    FleetTable t;
};
using FleetArgs = FleetArgsT<SqMesh>;
inline FleetArgsT<SqTiled> fleet_args_tiled(const FleetArgs& a) {
    return FleetArgsT<SqTiled>{SqTiled{a.m}, a.vel, a.iters, a.hull, a.tris, a.bodies, a.mass, a.wrench, a.vslab, a.part, a.rows, a.out, a.dt,
                               a.substeps, a.last, a.t};
}

// One lane per instance vertex of the table (k_hull_vertices per lane): slab row k is vertex `item` of body `body` of its hull.
template <typename Mesh>
__global__ __launch_bounds__(256) void k_fleet_vertices(FleetArgsT<Mesh> a) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.t.total[MW_FLEET_VERTS]) return;
    const FleetItem it = fleet_map(a.t, MW_FLEET_VERTS, (int)k);
    float body[16], h[3], s[8];
    // the hull vertex before the pose, and every table value before both: see "operand order" at the top of this file
    const float* vel = it.row.cf.drag ? a.vel : nullptr;
    const float vscale = it.row.vscale;
    for (int c = 0; c < 3; c++) h[c] = a.hull[3 * (size_t)(it.row.vert_first + it.item) + c];
    hull_load_body(a.bodies + 4 * (size_t)(it.row.body_first + it.body), body);
    hull_vertex(a.m, vel, vscale, a.iters, body, h, s);
    hull_store_row(a.vslab + 2 * k, s);
}

// One 256-lane workgroup per (body, chunk) of the table (k_hull_triangles per chunk); workgroups stride over them.
template <typename Mesh>
__global__ __launch_bounds__(256) void k_fleet_triangles(FleetArgsT<Mesh> a) {
    const int l = threadIdx.x;
    const int total = a.t.total[MW_FLEET_CHUNKS];
    for (int blk = blockIdx.x; blk < total; blk += gridDim.x) {
        const FleetItem it = fleet_map(a.t, MW_FLEET_CHUNKS, blk);
        const int nverts = it.row.nverts, ntris = it.row.ntris;
        const size_t b = (size_t)(it.row.body_first + it.body);
        const float* vs = reinterpret_cast<const float*>(a.vslab + 2 * ((size_t)it.row.first[MW_FLEET_VERTS] + (size_t)it.body * nverts));
        const int* tris = a.tris + 3 * (size_t)it.row.tri_first;
        float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        float res = 0.f;
        const int t = it.item * MW_HULL_CHUNK + l;
        if (t < ntris) {
            float body[16];
            hull_load_body(a.bodies + 4 * b, body);
            const int idx[3] = {tris[3 * (size_t)t], tris[3 * (size_t)t + 1], tris[3 * (size_t)t + 2]};
            if (!hull_triangle(idx, nverts, vs, body, it.row.cf, acc)) res = NAN;
        }
        if (t < nverts) res = hull_max(res, vs[8 * (size_t)t + 7]);
        hull_chunk_partial(acc, res, a.part + 2 * (size_t)blk);
    }
}

// One wave per body of the table (k_hull_reduce per wave): the row goes to rows[body] (fleet forces: rows is the call's out).
template <typename Mesh>
__global__ __launch_bounds__(256) void k_fleet_reduce(FleetArgsT<Mesh> a) {
    const int l = threadIdx.x & 63;
    const int64_t nwaves = (int64_t)gridDim.x * (blockDim.x >> 6);
    for (int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6; w < a.t.total[MW_FLEET_BODIES]; w += nwaves) {  // wave-uniform
        const FleetItem it = fleet_map(a.t, MW_FLEET_BODIES, (int)w);
        const int nchunks = it.row.nchunks;
        const size_t p = (size_t)it.row.first[MW_FLEET_CHUNKS] + (size_t)it.body * nchunks;
        float acc[7], res;
        hull_body_sum(a.part, p, nchunks, l, acc, res);
        if (l == 0) {
            float o[8];
            hull_row(acc, res, o);
            hull_store_row(a.rows + 2 * (size_t)(it.row.body_first + it.body), o);
        }
    }
}

// Per-substep plan, after the three kernels above: one lane per body of the table integrates its row (k_bodies_integrate per lane);
// the last substep also writes out.  Wrench is a template argument, not a branch on a.wrench: the kernel of a call without a wrench
// holds no trace of one, so that its body_integrate is k_bodies_integrate's operand for operand (see "operand order").
template <typename Mesh, bool Wrench>
__global__ __launch_bounds__(256) void k_fleet_integrate(FleetArgsT<Mesh> a) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= a.t.total[MW_FLEET_BODIES]) return;
    const FleetItem it = fleet_map(a.t, MW_FLEET_BODIES, (int)w);
    const size_t b = (size_t)(it.row.body_first + it.body);
    float body[16], mass[8], row[8], wr[8];
    hull_load_body(a.bodies + 4 * b, body);
    hull_load_row(a.mass + 2 * b, mass);
    hull_load_row(a.rows + 2 * b, row);
    bool valid = body_mass_valid(mass);
    if (Wrench) {
        hull_load_row(a.wrench + 2 * b, wr);
        valid = valid && fleet_wrench_valid(wr);
    }
    if (!valid) {
        for (int k = 0; k < 8; k++) row[k] = NAN;
    } else if (Wrench ? fleet_integrate(body, row, mass, wr, it.row.g, a.dt) : body_integrate(body, row, mass, it.row.g, a.dt)) {
        for (int k = 0; k < 4; k++) a.bodies[4 * b + k] = make_float4(body[4 * k], body[4 * k + 1], body[4 * k + 2], body[4 * k + 3]);
    }
    if (a.last && a.out) hull_store_row(a.out + 2 * b, row);
}

// One-launch plan: one 256-lane workgroup per body of the table runs every substep (k_bodies_step per workgroup), with the call's
// optional parts: the external wrench (a.wrench) and K mooring slots per body (lines [total_bodies][K][3], K == 0: none; tension
// [total_bodies][K] or nullptr).  The slots are staged once in LDS, and the tensions of the latest substep wait there for the end of the
// call.  Lane 0 ends a substep in one expression for every combination: the line wrench M of the state the row was evaluated at
// (mooring_wrench), then (F + W) + M, each add only when its part exists (fleet_pushed_row, fleet_integrate) -- moored_integrate on the
// row pushed by W.  No entry point passes a wrench and lines together.
// Dynamic LDS: the largest bodies_step_lds of the table's hulls; each workgroup lays out its own hull's slab and partials in it.
template <typename Mesh>
__global__ __launch_bounds__(MW_HULL_CHUNK) void k_fleet_step(FleetArgsT<Mesh> a, const float4* lines, float* tension, int K) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ float pose[16];
    __shared__ int stop;
    __shared__ __attribute__((aligned(16))) float slots[MW_MOORING_LINES * MW_MOORING_SLOT];
    __shared__ float tens[MW_MOORING_LINES];
    const FleetItem it = fleet_map(a.t, MW_FLEET_BODIES, (int)blockIdx.x);
    const int nverts = it.row.nverts, ntris = it.row.ntris, nchunks = it.row.nchunks;
    const float* hull = a.hull + 3 * (size_t)it.row.vert_first;
    const int* tris = a.tris + 3 * (size_t)it.row.tri_first;
    const float* vel = it.row.cf.drag ? a.vel : nullptr;
    float4* slab = reinterpret_cast<float4*>(smem);  // [nverts][2]
    float4* part = slab + 2 * (size_t)nverts;        // [nchunks][2]
    const float* vs = reinterpret_cast<const float*>(slab);
    const int l = threadIdx.x;
    const size_t b = (size_t)(it.row.body_first + it.body);
    float body[16], mass[8], row[8], wr[8];
    hull_load_body(a.bodies + 4 * b, body);
    hull_load_row(a.mass + 2 * b, mass);
    if (K > 0) {  // uniform over the launch
        if (l < 3 * K) reinterpret_cast<float4*>(slots)[l] = lines[3 * b * K + l];
        __syncthreads();
    }
    bool valid = body_mass_valid(mass);
    if (a.wrench) {
        hull_load_row(a.wrench + 2 * b, wr);
        valid = valid && fleet_wrench_valid(wr);
    }
    for (int s = 0; s < K; s++) valid = valid && mooring_slot_valid(slots + MW_MOORING_SLOT * s);
    if (!valid) {  // uniform over the workgroup
        for (int k = 0; k < 8; k++) row[k] = NAN;
        if (l == 0 && a.out) hull_store_row(a.out + 2 * b, row);
        if (l < K && tension) tension[b * K + l] = NAN;
        return;
    }
    for (int s = 0; s < a.substeps; s++) {
        // vertices (k_hull_vertices)
        for (int v = l; v < nverts; v += MW_HULL_CHUNK) {
            float h[3], sl[8];
            for (int c = 0; c < 3; c++) h[c] = hull[3 * (size_t)v + c];
            hull_vertex(a.m, vel, it.row.vscale, a.iters, body, h, sl);
            hull_store_row(slab + 2 * v, sl);
        }
        __syncthreads();
        // triangles (k_hull_triangles), chunk by chunk
        for (int c = 0; c < nchunks; c++) {
            float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            float res = 0.f;
            const int t = c * MW_HULL_CHUNK + l;
            if (t < ntris) {
                const int idx[3] = {tris[3 * (size_t)t], tris[3 * (size_t)t + 1], tris[3 * (size_t)t + 2]};
                if (!hull_triangle(idx, nverts, vs, body, it.row.cf, acc)) res = NAN;
            }
            if (t < nverts) res = hull_max(res, vs[8 * (size_t)t + 7]);
            hull_chunk_partial(acc, res, part + 2 * c);
        }
        // the row (k_hull_reduce), the line wrench and the integration, in wave 0
        if (l < 64) {
            float acc[7], res;
            hull_body_sum(part, 0, nchunks, l, acc, res);
            if (l == 0) {
                float pushed[8];
                hull_row(acc, res, row);
                fleet_pushed_row(row, a.wrench ? wr : nullptr, pushed);
                const bool ok = moored_integrate(body, pushed, mass, slots, K, it.row.g, a.dt, tens);
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
    if (l < K && tension) tension[b * K + l] = tens[l];  // lane 0 wrote tens before the loop's last barrier
}
#endif

}  // namespace mw
