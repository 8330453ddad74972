// tests/velocity_query_shim.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The MW_HD functions of the velocity feature compiled with g++ for the CPU tier (tests/test_velocity_cpu.py): the velocity query
// (sq_velocity_point in mistral-water_amd/csrc/surface_query.h, the code k_query_velocity runs per lane), the surface query it must
// locate identically to, the spectrum weighting (csrc/velocity_kernels.h) and the two dispersion relations whose mirror symmetry the
// weighted spectrum relies on.  Never part of libmistral_water.so and not a fallback.
//
// build: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared (tests/test_velocity_cpu.py)
#include <cstdint>

#include "../mistral-water_amd/csrc/ocean_renderer_kernels.h"
#include "../mistral-water_amd/csrc/surface_query.h"
#include "../mistral-water_amd/csrc/velocity_kernels.h"

using namespace mw;

extern "C" int vq_shim_query(int R, float unit_width, const float* vert, const float* vel, int mode, const float* xz, int64_t n, int iters,
                             float* out) {
    if (R < 2 || !(unit_width > 0.f) || iters < 0 || iters > MW_SQ_MAX_ITERS) return 1;
    SqMesh m{vert, vert, vert, R, 3, unit_width};  // normals / whitecap are not read by the velocity query
    for (int64_t k = 0; k < n; k++) sq_velocity_point(m, vel, mode, xz[2 * k], xz[2 * k + 1], iters == 0 ? MW_SQ_DEFAULT_ITERS : iters, out + 4 * k);
    return 0;
}

// omega_f32 (FFTMesh, S/FFTMesh.cs:141-147) over the N x N grid, [i][j]
extern "C" void vq_shim_omega(int N, float length, float gravity, float* out) {
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) out[i * N + j] = omega_f32(N, length, gravity, i, j);
}

// or_omega (OceanRenderer, F/FFTCommon.cginc:101-114) over the M x M texture, [px][py]
extern "C" void vq_shim_or_omega(int M, float length, float gravity, float* out) {
    OrConsts c{M, length, gravity, 0.f, length};
    for (int px = 0; px < M; px++)
        for (int py = 0; py < M; py++) out[px * M + py] = or_omega(c, px, py);
}

// velocity_weight over n complex pairs with per-element w
extern "C" void vq_shim_weight(const float* w, const float* h0, const float* h0c, int64_t n, float* va, float* vb) {
    for (int64_t k = 0; k < n; k++) {
        cf a, b;
        velocity_weight(w[k], mk(h0[2 * k], h0[2 * k + 1]), mk(h0c[2 * k], h0c[2 * k + 1]), &a, &b);
        va[2 * k] = a.x; va[2 * k + 1] = a.y; vb[2 * k] = b.x; vb[2 * k + 1] = b.y;
    }
}
