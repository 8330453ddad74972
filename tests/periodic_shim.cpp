// tests/periodic_shim.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The MW_HD functions of the surface services (mistral-water_amd/csrc/surface_query.h, hull_forces.h, rigid_bodies.h) compiled with g++
// over a mesh read as its infinite tiling (SqTiled, period != 0) or as the one footprint (SqMesh, period == 0): the surface and velocity
// queries, the hull vertex step, the rows summed in the kernels' own order, and the substep chain of the bodies in both plans' order.
// The tiled kernels are built without floating-point contraction (csrc/surface_tiled.hip), so what this file computes for period != 0 is
// what the device computes, bit for bit (tests/test_periodic_gpu.py).  Never part of libmistral_water.so and not a fallback.
//
// build: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared (tests/test_periodic_cpu.py)
#include <cstdint>
#include <vector>

#include "../mistral-water_amd/csrc/rigid_bodies.h"

using namespace mw;

namespace {
SqMesh mesh_of(int R, float uw, float period, const float* vert, const float* norm, const float* white, int wstride) {
    SqMesh m{vert, norm, white, R, wstride, uw};
    m.period = period;
    return m;
}
bool bad(int R, float uw, int iters) { return R < 2 || !(uw > 0.f) || iters < 0 || iters > MW_SQ_MAX_ITERS; }
int its(int iters) { return iters == 0 ? MW_SQ_DEFAULT_ITERS : iters; }

// lane 0 of the kernels' shuffle tree over 64 lanes: v[l] (+)= v[l + off], off = 32 ... 1 (only the lanes that reach lane 0 are kept)
void tree(float acc[64][7], float res[64]) {
    for (int off = 32; off > 0; off >>= 1)
        for (int l = 0; l < off; l++) {
            for (int k = 0; k < 7; k++) acc[l][k] += acc[l + off][k];
            res[l] = hull_max(res[l], res[l + off]);
        }
}

// the row of one body from its vertex slab vs [nverts][8], summed as k_hull_triangles and k_hull_reduce (and k_bodies_step) sum it:
// 256-triangle chunks, a tree per wave, the four waves in order, the chunks of a lane in order, the lane tree
void body_row(const int* tris, int ntris, int nverts, const float* vs, const float body[16], const HullCoeffs& cf, float row[8]) {
    const int nchunks = ((ntris > nverts ? ntris : nverts) + MW_HULL_CHUNK - 1) / MW_HULL_CHUNK;
    std::vector<float> part((size_t)nchunks * 8);
    for (int c = 0; c < nchunks; c++) {
        float o[8];
        for (int w = 0; w < MW_HULL_CHUNK / 64; w++) {
            float acc[64][7], res[64];
            for (int lane = 0; lane < 64; lane++) {
                for (int k = 0; k < 7; k++) acc[lane][k] = 0.f;
                res[lane] = 0.f;
                const int t = c * MW_HULL_CHUNK + w * 64 + lane;
                if (t < ntris && !hull_triangle(tris + 3 * (size_t)t, nverts, vs, body, cf, acc[lane])) res[lane] = NAN;
                if (t < nverts) res[lane] = hull_max(res[lane], vs[8 * (size_t)t + 7]);
            }
            tree(acc, res);
            if (w == 0) {
                for (int k = 0; k < 7; k++) o[k] = acc[0][k];
                o[7] = res[0];
            } else {
                for (int k = 0; k < 7; k++) o[k] += acc[0][k];
                o[7] = hull_max(o[7], res[0]);
            }
        }
        for (int k = 0; k < 8; k++) part[8 * (size_t)c + k] = o[k];
    }
    float acc[64][7], res[64];
    for (int l = 0; l < 64; l++) {
        for (int k = 0; k < 7; k++) acc[l][k] = 0.f;
        res[l] = 0.f;
        for (int c = l; c < nchunks; c += 64) {
            for (int k = 0; k < 7; k++) acc[l][k] += part[8 * (size_t)c + k];
            res[l] = hull_max(res[l], part[8 * (size_t)c + 7]);
        }
    }
    tree(acc, res);
    hull_row(acc[0], res[0], row);
}

template <typename Mesh>
void vertices(const Mesh& m, const float* vel, float vscale, int iters, const float* hull, int nverts, const float body[16], float* slab) {
    for (int v = 0; v < nverts; v++) hull_vertex(m, vel, vscale, iters, body, hull + 3 * v, slab + 8 * (size_t)v);
}

struct Call {
    const float *vel, *hull; const int* tris; int nverts, ntris; float vscale; int iters; HullCoeffs cf; float g, h; int substeps;
};

// mw_ocean_step_bodies in the order of each plan (csrc/rigid_bodies.h): 0 per substep (every body's row, then every body's integration),
// 1 one launch (a body runs all its substeps, stopping at a NaN row)
template <typename Mesh>
void step_bodies(const Mesh& m, const Call& c, int plan, float* bodies, const float* mass, int nbodies, float* out) {
    std::vector<float> slab((size_t)c.nverts * 8), rows((size_t)nbodies * 8);
    if (plan == 0) {
        for (int s = 0; s < c.substeps; s++) {
            for (int b = 0; b < nbodies; b++) {
                vertices(m, c.vel, c.vscale, c.iters, c.hull, c.nverts, bodies + 16 * b, slab.data());
                body_row(c.tris, c.ntris, c.nverts, slab.data(), bodies + 16 * b, c.cf, rows.data() + 8 * b);
            }
            for (int b = 0; b < nbodies; b++) {
                float* row = rows.data() + 8 * b;
                if (!body_mass_valid(mass + 8 * b)) {
                    for (int k = 0; k < 8; k++) row[k] = NAN;
                } else {
                    body_integrate(bodies + 16 * b, row, mass + 8 * b, c.g, c.h);
                }
                if (s == c.substeps - 1 && out)
                    for (int k = 0; k < 8; k++) out[8 * b + k] = row[k];
            }
        }
        return;
    }
    for (int b = 0; b < nbodies; b++) {
        float row[8];
        if (!body_mass_valid(mass + 8 * b)) {
            if (out)
                for (int k = 0; k < 8; k++) out[8 * b + k] = NAN;
            continue;
        }
        for (int s = 0; s < c.substeps; s++) {
            vertices(m, c.vel, c.vscale, c.iters, c.hull, c.nverts, bodies + 16 * b, slab.data());
            body_row(c.tris, c.ntris, c.nverts, slab.data(), bodies + 16 * b, c.cf, row);
            if (!body_integrate(bodies + 16 * b, row, mass + 8 * b, c.g, c.h)) break;
        }
        if (out)
            for (int k = 0; k < 8; k++) out[8 * b + k] = row[k];
    }
}
}  // namespace

// P = (float)N * unit_width and the rest coordinate of grid line g of the tiling
extern "C" float ps_period(int N, float unit_width) { return (float)N * unit_width; }
extern "C" float ps_rest(int N, float unit_width, int g) { return sq_tiled_rest(N, unit_width, (float)N * unit_width, g); }

// the launch arithmetic of a hull call: its chunks, the dynamic LDS of the one-launch plan and that plan's limit
extern "C" int ps_hull_chunks(int nverts, int ntris) { return hull_chunks(nverts, ntris); }
extern "C" int64_t ps_bodies_step_lds(int nverts, int nchunks) { return (int64_t)bodies_step_lds(nverts, nchunks); }
extern "C" int64_t ps_bodies_lds_max() { return MW_BODIES_LDS_MAX; }

// sq_query_point over n points; period == 0: the one footprint
extern "C" int ps_query(int R, float unit_width, float period, const float* vert, const float* norm, const float* white, int wstride, int mode,
                        const float* xz, int64_t n, int iters, float* out) {
    if (bad(R, unit_width, iters)) return 1;
    const SqMesh m = mesh_of(R, unit_width, period, vert, norm, white, wstride);
    for (int64_t k = 0; k < n; k++) {
        if (period != 0.f) sq_query_point(SqTiled{m}, mode, xz[2 * k], xz[2 * k + 1], its(iters), out + 8 * k);
        else sq_query_point(m, mode, xz[2 * k], xz[2 * k + 1], its(iters), out + 8 * k);
    }
    return 0;
}

// sq_velocity_point over n points
extern "C" int ps_velocity(int R, float unit_width, float period, const float* vert, const float* vel, int mode, const float* xz, int64_t n,
                           int iters, float* out) {
    if (bad(R, unit_width, iters)) return 1;
    const SqMesh m = mesh_of(R, unit_width, period, vert, vert, vert, 3);  // normals / whitecap are not read
    for (int64_t k = 0; k < n; k++) {
        if (period != 0.f) sq_velocity_point(SqTiled{m}, vel, mode, xz[2 * k], xz[2 * k + 1], its(iters), out + 4 * k);
        else sq_velocity_point(m, vel, mode, xz[2 * k], xz[2 * k + 1], its(iters), out + 4 * k);
    }
    return 0;
}

// coeffs = (density, gravity, linear_drag, quadratic_drag, velocity_scale), as mw_ocean_hull_forces takes them.
// slab [nbodies][nverts][8] (hull_vertex) and rows [nbodies][8] in the kernels' summation order; vel may be NULL (drag off)
extern "C" int ps_hull_forces(int R, float unit_width, float period, const float* vert, const float* vel, int iters, const float* hull, int nverts,
                              const int* tris, int ntris, const float* bodies, int nbodies, const float* coeffs, float* slab, float* rows) {
    if (bad(R, unit_width, iters)) return 1;
    const SqMesh m = mesh_of(R, unit_width, period, vert, vert, vert, 3);
    HullCoeffs cf;
    float g, vscale;
    hull_coeffs(coeffs, &cf, &g, &vscale);
    const float* u = cf.drag ? vel : nullptr;
    for (int b = 0; b < nbodies; b++) {
        float* s = slab + 8 * (size_t)b * nverts;
        if (period != 0.f) vertices(SqTiled{m}, u, vscale, its(iters), hull, nverts, bodies + 16 * b, s);
        else vertices(m, u, vscale, its(iters), hull, nverts, bodies + 16 * b, s);
        body_row(tris, ntris, nverts, s, bodies + 16 * b, cf, rows + 8 * b);
    }
    return 0;
}

// mw_ocean_step_bodies: bodies [nbodies][16] in place, out [nbodies][8] or NULL; plan 0 per substep, 1 one launch
extern "C" int ps_step_bodies(int R, float unit_width, float period, const float* vert, const float* vel, int iters, const float* hull, int nverts,
                              const int* tris, int ntris, float* bodies, const float* mass, int nbodies, const float* coeffs, float dt,
                              int substeps, int plan, float* out) {
    if (bad(R, unit_width, iters) || substeps < 1) return 1;
    const SqMesh m = mesh_of(R, unit_width, period, vert, vert, vert, 3);
    HullCoeffs cf;
    float g, vscale;
    hull_coeffs(coeffs, &cf, &g, &vscale);
    const Call c{cf.drag ? vel : nullptr, hull, tris, nverts, ntris, vscale, its(iters), cf, g, dt / (float)substeps, substeps};
    if (period != 0.f) step_bodies(SqTiled{m}, c, plan, bodies, mass, nbodies, out);
    else step_bodies(m, c, plan, bodies, mass, nbodies, out);
    return 0;
}
