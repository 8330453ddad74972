// tests/surface_query_shim.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The MW_HD functions of mistral-water_amd/csrc/surface_query.h -- the very code k_query_surface runs per lane -- compiled with
// g++ so that the CPU test tier (tests/test_surface_query_cpu.py) can check the point-in-triangle, affine-solve and walk logic
// against a numpy brute-force reference without a GPU.  Never part of libmistral_water.so and not a fallback.
//
// build: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared (tests/test_surface_query_cpu.py)
#include <cstdint>

#include "../mistral-water_amd/csrc/surface_query.h"

using namespace mw;

extern "C" int sq_shim_query(int R, float unit_width, const float* vert, const float* norm, const float* white, int wstride, int mode,
                             const float* xz, int64_t n, int iters, float* out) {
    if (R < 2 || !(unit_width > 0.f) || iters < 0 || iters > MW_SQ_MAX_ITERS) return 1;
    SqMesh m{vert, norm, white, R, wstride, unit_width};
    for (int64_t k = 0; k < n; k++) sq_query_point(m, mode, xz[2 * k], xz[2 * k + 1], iters == 0 ? MW_SQ_DEFAULT_ITERS : iters, out + 8 * k);
    return 0;
}

extern "C" float sq_shim_rest_coord(int R, float unit_width, int a) { return rest_coord(R, unit_width, a); }
