// tests/raycast_tiled_shim.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The MW_HD functions of mistral-water_amd/csrc/raycast_tiled.h -- the wrapped hierarchy, the column walk and the instance traversal
// k_raycast_tiled runs per lane -- compiled with g++ so that the CPU tier (tests/test_raycast_tiled_cpu.py) can hold the walk against a
// brute force over every triangle of every window tile, and the GPU tier (tests/test_raycast_tiled_gpu.py) the device against this
// build, bit for bit.  Never part of libmistral_water.so and not a fallback.
//
// build: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared (tests/ray_tiled_ref.py)
#include <cstdint>
#include <vector>

#include "../mistral-water_amd/csrc/raycast_tiled.h"

using namespace mw;

static SqMesh mesh_of(int N, float uw, float P, const float* vert, const float* norm, const float* white, int wstride) {
    SqMesh m{vert, norm, white, N, wstride, uw, P};
    return m;
}
static bool bad(int N, float P, int B, int reach) { return N < 2 || !(P > 0.f) || B < 1 || reach < 0 || reach > MW_RCT_MAX_REACH; }

extern "C" int rct_shim_max_reach() { return MW_RCT_MAX_REACH; }

extern "C" int64_t rct_shim_nodes(int N, int B) { return rc_nodes(rct_tree(nullptr, N, B).D); }

// the hierarchy of one tile into box [rct_shim_nodes(N, B)][8]
extern "C" int rct_shim_build(int N, float uw, float P, const float* vert, int B, float* box) {
    if (bad(N, P, B, 0)) return 1;
    rct_build_serial(mesh_of(N, uw, P, vert, nullptr, nullptr, 1), rct_tree(box, N, B));
    return 0;
}

// the root box (lo.x lo.y lo.z hi.x hi.y hi.z), the footprint's lower corner x0 and h, the tiles a tile's geometry can overhang
extern "C" int rct_shim_root(int N, float uw, float P, const float* vert, int B, float* root6, float* x0, int32_t* h) {
    if (bad(N, P, B, 0)) return 1;
    std::vector<float> box((size_t)rct_shim_nodes(N, B) * 8);
    rct_shim_build(N, uw, P, vert, B, box.data());
    rc_load_box(box.data(), 0, root6, root6 + 3);
    *x0 = rest_coord(N, uw, 0);
    *h = rct_overhang_tiles(root6, root6 + 3, *x0, P);
    return 0;
}

// h of a root box (lo.x lo.y lo.z hi.x hi.y hi.z) somebody else built
extern "C" int rct_shim_overhang(int N, float uw, float P, const float* root6) {
    return rct_overhang_tiles(root6, root6 + 3, rest_coord(N, uw, 0), P);
}

// build, then the column walk -> out [n][8], hit [n][4]
extern "C" int rct_shim_cast(int N, float uw, float P, const float* vert, const float* norm, const float* white, int wstride, int B,
                             int reach, const float* rays, int64_t n, float* out, int32_t* hit) {
    if (bad(N, P, B, reach)) return 1;
    std::vector<float> box((size_t)rct_shim_nodes(N, B) * 8);
    rct_shim_build(N, uw, P, vert, B, box.data());
    const SqMesh m = mesh_of(N, uw, P, vert, norm, white, wstride);
    const RcTree t = rct_tree(box.data(), N, B);
    for (int64_t k = 0; k < n; k++) rct_cast(m, t, rays + 8 * k, reach, out + 8 * k, hit + 4 * k);
    return 0;
}

// every triangle of every window tile for every ray, the same intersection and tie rule
extern "C" int rct_shim_brute(int N, float uw, float P, const float* vert, const float* norm, const float* white, int wstride, int reach,
                              const float* rays, int64_t n, float* out, int32_t* hit) {
    if (bad(N, P, 1, reach)) return 1;
    const SqMesh m = mesh_of(N, uw, P, vert, norm, white, wstride);
    for (int64_t k = 0; k < n; k++) rct_cast_brute(m, rays + 8 * k, reach, out + 8 * k, hit + 4 * k);
    return 0;
}
