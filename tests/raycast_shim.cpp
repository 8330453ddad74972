// tests/raycast_shim.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The MW_HD functions of mistral-water_amd/csrc/raycast.h -- the intersection, hierarchy and traversal k_raycast runs per lane --
// compiled with g++ so that the CPU tier (tests/test_raycast_cpu.py) can hold the traversal against a brute force over every triangle,
// and the GPU tier (tests/test_raycast_gpu.py) the device against this build, bit for bit.  Never part of libmistral_water.so and not a
// fallback.
//
// build: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared (tests/ray_ref.py)
#include <cstdint>
#include <vector>

#include "../mistral-water_amd/csrc/raycast.h"

using namespace mw;

static SqMesh mesh_of(int R, float uw, const float* vert, const float* norm, const float* white, int wstride) {
    SqMesh m{vert, norm, white, R, wstride, uw};
    return m;
}

extern "C" int rc_shim_default_block() { return MW_RC_DEFAULT_BLOCK; }

extern "C" int64_t rc_shim_nodes(int R, int B) { return rc_nodes(rc_tree(nullptr, R, B).D); }

// the hierarchy of the mesh into box [rc_shim_nodes(R, B)][8]
extern "C" int rc_shim_build(int R, const float* vert, int B, float* box) {
    if (R < 2 || B < 1) return 1;
    rc_build_serial(mesh_of(R, 1.f, vert, nullptr, nullptr, 1), rc_tree(box, R, B));
    return 0;
}

// rays [n][8] through a hierarchy rc_shim_build made -> out [n][8], hit [n][2]
extern "C" int rc_shim_trace(int R, const float* vert, const float* norm, const float* white, int wstride, int B, const float* box,
                             const float* rays, int64_t n, float* out, int32_t* hit) {
    if (R < 2 || B < 1) return 1;
    const SqMesh m = mesh_of(R, 1.f, vert, norm, white, wstride);
    const RcTree t = rc_tree(const_cast<float*>(box), R, B);
    for (int64_t k = 0; k < n; k++) rc_cast(m, t, rays + 8 * k, out + 8 * k, hit + 2 * k);
    return 0;
}

// build, then trace
extern "C" int rc_shim_cast(int R, const float* vert, const float* norm, const float* white, int wstride, int B, const float* rays,
                            int64_t n, float* out, int32_t* hit) {
    if (R < 2 || B < 1) return 1;
    std::vector<float> box((size_t)rc_shim_nodes(R, B) * 8);
    rc_shim_build(R, vert, B, box.data());
    return rc_shim_trace(R, vert, norm, white, wstride, B, box.data(), rays, n, out, hit);
}

// every triangle for every ray, the same intersection and tie rule
extern "C" int rc_shim_brute(int R, const float* vert, const float* norm, const float* white, int wstride, const float* rays, int64_t n,
                             float* out, int32_t* hit) {
    if (R < 2) return 1;
    const SqMesh m = mesh_of(R, 1.f, vert, norm, white, wstride);
    for (int64_t k = 0; k < n; k++) rc_cast_brute(m, rays + 8 * k, out + 8 * k, hit + 2 * k);
    return 0;
}

// world-mode surface queries (sq_query_point) -> out [n][8], and the id of the triangle sq_locate names for each (-1: none)
extern "C" int rc_shim_query_world(int R, float uw, const float* vert, const float* norm, const float* white, int wstride, const float* xz,
                                   int64_t n, int iters, float* out, int32_t* tri) {
    if (R < 2 || iters < 1 || iters > MW_SQ_MAX_ITERS) return 1;
    const SqMesh m = mesh_of(R, uw, vert, norm, white, wstride);
    for (int64_t k = 0; k < n; k++) {
        sq_query_point(m, MW_SQ_WORLD, xz[2 * k], xz[2 * k + 1], iters, out + 8 * k);
        tri[k] = -1;
        sq_locate(m, MW_SQ_WORLD, xz[2 * k], xz[2 * k + 1], iters, [] {}, [&](const int v[3], const float*) {
            const int c00 = v[2] - 1;  // corner (i, j+1) is the last of both triangles
            tri[k] = 2 * ((c00 / R) * (R - 1) + c00 % R) + (v[0] != c00 ? 1 : 0);
        });
    }
    return 0;
}
