// tests/hull_order.h -- TEST INFRASTRUCTURE ONLY.
//
// The order in which the hull family sums a body's row and steps its bodies, restated by hand: this header is
// the one oracle for that order, included by periodic_shim.cpp and draught_shim.cpp, which differ in the vertex step alone and hand it
// in as a callable.  It calls the per-item MW_HD functions (hull_triangle, hull_max, hull_row, body_integrate, body_mass_valid) and
// none of the device code's own sums, so a change of order there shows as a mismatch here.
#pragma once
#include <cstddef>
#include <vector>

#include "../mistral-water_amd/csrc/rigid_bodies.h"

namespace hull_order {
using namespace mw;

// lane 0 of the shuffle tree of one wave: v[l] (+)= v[l + off], off = 32 ... 1 (only the lanes that reach lane 0 are kept)
inline void tree(float acc[64][7], float res[64]) {
    for (int off = 32; off > 0; off >>= 1)
        for (int l = 0; l < off; l++) {
            for (int k = 0; k < 7; k++) acc[l][k] += acc[l + off][k];
            res[l] = hull_max(res[l], res[l + off]);
        }
}

// The row of one body from its vertex slab vs [nverts][8]: chunks of 256 triangles and vertices; in a chunk lane l holds triangle
// c * 256 + l and the residual of vertex c * 256 + l; a tree per wave of 64 lanes; the four waves added in wave order; then lane l of
// one wave adds the chunks l, l + 64, ... in order, and a last tree.
inline void body_row(const int* tris, int ntris, int nverts, const float* vs, const float body[16], const HullCoeffs& cf, float row[8]) {
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

// what the row and the substeps of a call take besides the vertex step
struct Call {
    const int* tris; int nverts, ntris; HullCoeffs cf; float g, h; int substeps;  // h = dt / substeps
};

// vertices(body, slab) writes the vertex slab [nverts][8] of one body; its row follows
template <typename Vertices>
void forces(const Call& c, Vertices vertices, const float body[16], float* slab, float row[8]) {
    vertices(body, slab);
    body_row(c.tris, c.ntris, c.nverts, slab, body, c.cf, row);
}

// mw_ocean_step_bodies in the order of each plan (csrc/rigid_bodies.h): 0 per substep (every body's row, then every body's integration),
// 1 one launch (a body runs all its substeps, stopping at a NaN row).  bodies [nbodies][16] in place, out [nbodies][8] or NULL.
template <typename Vertices>
void step_bodies(const Call& c, Vertices vertices, int plan, float* bodies, const float* mass, int nbodies, float* out) {
    std::vector<float> slab((size_t)c.nverts * 8), rows((size_t)nbodies * 8);
    if (plan == 0) {
        for (int s = 0; s < c.substeps; s++) {
            for (int b = 0; b < nbodies; b++) forces(c, vertices, bodies + 16 * b, slab.data(), rows.data() + 8 * b);
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
            forces(c, vertices, bodies + 16 * b, slab.data(), row);
            if (!body_integrate(bodies + 16 * b, row, mass + 8 * b, c.g, c.h)) break;
        }
        if (out)
            for (int k = 0; k < 8; k++) out[8 * b + k] = row[k];
    }
}
}  // namespace hull_order
