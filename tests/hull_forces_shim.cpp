// tests/hull_forces_shim.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The MW_HD functions of the hull-forces feature (mistral-water_amd/csrc/hull_forces.h) compiled with g++ for the CPU tier
// (tests/test_hull_forces_cpu.py): the vertex step k_hull_vertices runs per lane (pose, the world-mode walk, height, velocity,
// residual) and the triangle step k_hull_triangles runs per lane (clip, pressure integrals, drag), on host arrays.  Never part of
// libmistral_water.so and not a fallback.
//
// build: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared (tests/test_hull_forces_cpu.py)
#include <cstdint>

#include "../mistral-water_amd/csrc/hull_forces.h"

using namespace mw;

// the kernels' coefficients, as the library derives them from the ABI's five (velocity_scale is not read here)
static HullCoeffs coeffs_of(float density, float gravity, float linear_drag, float quadratic_drag) {
    const float k[5] = {density, gravity, linear_drag, quadratic_drag, 1.f};
    HullCoeffs cf;
    float g, vscale;
    hull_coeffs(k, &cf, &g, &vscale);
    return cf;
}

// slab [nbodies][nverts][8] of hull_vertex over a synthetic mesh vert [R*R][3] (vel [R*R][3] or NULL: drag off)
extern "C" int hs_vertices(int R, float unit_width, const float* vert, const float* vel, float vscale, int iters, const float* hull,
                           int nverts, const float* bodies, int nbodies, float* slab) {
    if (R < 2 || !(unit_width > 0.f) || iters < 0 || iters > MW_SQ_MAX_ITERS) return 1;
    SqMesh m{vert, vert, vert, R, 3, unit_width};  // normals / whitecap are not read
    for (int b = 0; b < nbodies; b++)
        for (int v = 0; v < nverts; v++)
            hull_vertex(m, vel, vscale, iters == 0 ? MW_SQ_DEFAULT_ITERS : iters, bodies + 16 * b, hull + 3 * v,
                        slab + 8 * ((size_t)b * nverts + v));
    return 0;
}

// terms [nbodies][ntris][8] of hull_triangle: (Fx, Fy, Fz, area, tx, ty, tz, ok) per triangle, ok = 0 for a bad index
extern "C" void hs_triangles(const int* tris, int ntris, int nverts, const float* slab, const float* bodies, int nbodies, float density,
                             float gravity, float linear_drag, float quadratic_drag, float* terms) {
    const HullCoeffs cf = coeffs_of(density, gravity, linear_drag, quadratic_drag);
    for (int b = 0; b < nbodies; b++)
        for (int t = 0; t < ntris; t++) {
            float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            const bool ok = hull_triangle(tris + 3 * t, nverts, slab + 8 * (size_t)b * nverts, bodies + 16 * b, cf, acc);
            float* o = terms + 8 * ((size_t)b * ntris + t);
            for (int k = 0; k < 7; k++) o[k] = acc[k];
            o[7] = ok ? 1.f : 0.f;
        }
}

// sub-triangles of hull_clip for corners given as (x y z d ux uy uz) x 3: returns the count, sub [2][3][7]
extern "C" int hs_clip(const float* in, float* sub) {
    HullCorner c[3];
    for (int k = 0; k < 3; k++) {
        for (int i = 0; i < 3; i++) { c[k].x[i] = in[7 * k + i]; c[k].u[i] = in[7 * k + 4 + i]; }
        c[k].d = in[7 * k + 3];
    }
    int n = 0;
    return hull_clip(c[0], c[1], c[2], [&](const HullCorner& a, const HullCorner& b, const HullCorner& e) {
        const HullCorner* s[3] = {&a, &b, &e};
        for (int k = 0; k < 3; k++) {
            float* o = sub + 21 * n + 7 * k;
            for (int i = 0; i < 3; i++) { o[i] = s[k]->x[i]; o[4 + i] = s[k]->u[i]; }
            o[3] = s[k]->d;
        }
        n++;
    });
}

// rows [nbodies][8] from the slab: hull_triangle over the triangles and the NaN-propagating max residual over the vertices, summed in
// index order (the kernels sum the same terms in a fixed tree order), then hull_row -- the NaN rule of the output
extern "C" void hs_rows(const int* tris, int ntris, int nverts, const float* slab, const float* bodies, int nbodies, float density,
                        float gravity, float linear_drag, float quadratic_drag, float* rows) {
    const HullCoeffs cf = coeffs_of(density, gravity, linear_drag, quadratic_drag);
    for (int b = 0; b < nbodies; b++) {
        const float* vs = slab + 8 * (size_t)b * nverts;
        float acc[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, res = 0.f;
        for (int t = 0; t < ntris; t++)
            if (!hull_triangle(tris + 3 * t, nverts, vs, bodies + 16 * b, cf, acc)) res = NAN;
        for (int v = 0; v < nverts; v++) res = hull_max(res, vs[8 * v + 7]);
        hull_row(acc, res, rows + 8 * b);
    }
}
