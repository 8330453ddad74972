// tests/draught_shim.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The MW_HD functions of the hull family with draught on (mistral-water_amd/csrc/hull_draught.h over water_column.h, hull_forces.h and
// rigid_bodies.h) compiled with g++ over given layer arrays, read as the one footprint (period == 0) or as their tiling (period != 0):
// the vertex step on the column, the rows summed in the kernels' own order -- restated here by hand: this file is the oracle for that
// order -- and the substep chain.  The draught kernels are built without floating-point contraction (csrc/water_column.hip), so what this
// file computes is what the device computes on the same layer arrays, bit for bit (tests/test_draught_gpu.py).  Never part of
// libmistral_water.so and not a fallback.
//
// build: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared (tests/draught_ref.py::build_shim)
#include <cstdint>
#include <vector>

#include "../mistral-water_amd/csrc/hull_draught.h"
#include "../mistral-water_amd/csrc/water_column.h"
#include "../mistral-water_amd/csrc/rigid_bodies.h"

using namespace mw;

namespace {
// lane 0 of the shuffle tree of one wave: v[l] (+)= v[l + off], off = 32 ... 1
void tree(float acc[64][7], float res[64]) {
    for (int off = 32; off > 0; off >>= 1)
        for (int l = 0; l < off; l++) {
            for (int k = 0; k < 7; k++) acc[l][k] += acc[l + off][k];
            res[l] = hull_max(res[l], res[l + off]);
        }
}

// The row of one body from its vertex slab vs [nverts][8], in the order of DESIGN.md section 7d: chunks of 256 triangles and vertices;
// in a chunk lane l holds triangle c * 256 + l and the residual of vertex c * 256 + l; a tree per wave of 64 lanes; the four waves added
// in wave order; then lane l of one wave adds the chunks l, l + 64, ... in order, and a last tree.
void body_row(const int* tris, int ntris, int nverts, const float* vs, const float body[16], const HullCoeffs& cf, float row[8]) {
    const int most = ntris > nverts ? ntris : nverts;
    const int nchunks = (most + 255) / 256;
    std::vector<float> part((size_t)nchunks * 8);
    for (int c = 0; c < nchunks; c++) {
        float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int w = 0; w < 4; w++) {
            float acc[64][7], res[64];
            for (int lane = 0; lane < 64; lane++) {
                for (int k = 0; k < 7; k++) acc[lane][k] = 0.f;
                res[lane] = 0.f;
                const int t = c * 256 + w * 64 + lane;
                if (t < ntris && !hull_triangle(tris + 3 * (size_t)t, nverts, vs, body, cf, acc[lane])) res[lane] = NAN;
                if (t < nverts) res[lane] = hull_max(res[lane], vs[8 * (size_t)t + 7]);
            }
            tree(acc, res);
            for (int k = 0; k < 7; k++) o[k] = w == 0 ? acc[0][k] : o[k] + acc[0][k];
            o[7] = w == 0 ? res[0] : hull_max(o[7], res[0]);
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

struct Call {
    SqMesh m; ColTable tb; const float* hull; const int* tris; int nverts, ntris; float vscale; int iters; HullCoeffs cf; float g;
};

// fills c from the arguments every export takes; false: bad arguments
bool call_of(int R, float uw, float period, int L, const float* depths, const float* pos, const float* vel, int iters, const float* hull, int nverts,
             const int* tris, int ntris, const float* coeffs, Call* c) {
    if (R < 2 || !(uw > 0.f) || L < 2 || L > MW_COL_MAX_LAYERS || iters < 0 || iters > MW_SQ_MAX_ITERS) return false;
    c->m = SqMesh{nullptr, nullptr, nullptr, R, 1, uw};
    c->m.period = period;
    c->tb = ColTable{};
    c->tb.L = L;
    for (int l = 0; l < L; l++) {
        c->tb.depth[l] = depths[l];
        c->tb.pos[l] = pos + (size_t)l * R * R * 3;
        c->tb.vel[l] = vel + (size_t)l * R * R * 3;
    }
    c->m.vert = c->tb.pos[0];
    c->hull = hull; c->tris = tris; c->nverts = nverts; c->ntris = ntris;
    c->iters = iters == 0 ? MW_SQ_DEFAULT_ITERS : iters;
    hull_coeffs(coeffs, &c->cf, &c->g, &c->vscale);
    return true;
}

// the vertex slab of one body [nverts][8] and its row
void forces_of(const Call& c, const float body[16], float* slab, float row[8]) {
    for (int v = 0; v < c.nverts; v++) {
        if (c.m.period != 0.f) hull_vertex_draught(SqTiled{c.m}, c.tb, c.cf.drag, c.vscale, c.iters, body, c.hull + 3 * v, slab + 8 * (size_t)v);
        else hull_vertex_draught(c.m, c.tb, c.cf.drag, c.vscale, c.iters, body, c.hull + 3 * v, slab + 8 * (size_t)v);
    }
    body_row(c.tris, c.ntris, c.nverts, slab, body, c.cf, row);
}
}  // namespace

extern "C" {

// pos, vel: [L][R*R][3] contiguous (pos[0] the surface mesh, vel[0] the surface velocity); period == 0: the one footprint.
// coeffs = (density, gravity, linear_drag, quadratic_drag, velocity_scale).  slab [nbodies][nverts][8], rows [nbodies][8].  -1: bad arguments
int ds_hull_forces(int R, float uw, float period, int L, const float* depths, const float* pos, const float* vel, int iters, const float* hull,
                   int nverts, const int* tris, int ntris, const float* bodies, int nbodies, const float* coeffs, float* slab, float* rows) {
    Call c;
    if (!call_of(R, uw, period, L, depths, pos, vel, iters, hull, nverts, tris, ntris, coeffs, &c)) return -1;
    for (int b = 0; b < nbodies; b++) forces_of(c, bodies + 16 * b, slab + 8 * (size_t)b * nverts, rows + 8 * b);
    return 0;
}

// mw_ocean_step_bodies with draught on: per substep every body's row, then every body's integration; bodies [nbodies][16] in place,
// out [nbodies][8] (the rows of the last substep) or NULL
int ds_step_bodies(int R, float uw, float period, int L, const float* depths, const float* pos, const float* vel, int iters, const float* hull,
                   int nverts, const int* tris, int ntris, float* bodies, const float* mass, int nbodies, const float* coeffs, float dt, int substeps,
                   float* out) {
    Call c;
    if (!call_of(R, uw, period, L, depths, pos, vel, iters, hull, nverts, tris, ntris, coeffs, &c) || substeps < 1) return -1;
    const float h = dt / (float)substeps;
    std::vector<float> slab((size_t)nverts * 8), rows((size_t)nbodies * 8);
    for (int s = 0; s < substeps; s++) {
        for (int b = 0; b < nbodies; b++) forces_of(c, bodies + 16 * b, slab.data(), rows.data() + 8 * b);
        for (int b = 0; b < nbodies; b++) {
            float* row = rows.data() + 8 * b;
            if (!body_mass_valid(mass + 8 * b)) {
                for (int k = 0; k < 8; k++) row[k] = NAN;
            } else {
                body_integrate(bodies + 16 * b, row, mass + 8 * b, c.g, h);
            }
            if (s == substeps - 1 && out)
                for (int k = 0; k < 8; k++) out[8 * b + k] = row[k];
        }
    }
    return 0;
}

}  // extern "C"
