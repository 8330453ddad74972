// tests/fleet_shim.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The MW_HD functions of the mixed-fleet feature (mistral-water_amd/csrc/fleet.h) compiled with g++ for the CPU tier
// (tests/test_fleet_cpu.py): the hull table and its work mapping, the wrench step and the wrench-row check, on host arrays.  Never part
// of libmistral_water.so and not a fallback.
//
// build: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared (tests/test_fleet_cpu.py)
#include <cstdint>

#include "../mistral-water_amd/csrc/fleet.h"

using namespace mw;

// the chunks of one hull of a table
extern "C" int fs_chunks(int nverts, int ntris) { return fleet_chunks(nverts, ntris); }

// fleet_table of hulls [nhulls][5] with the hulls of `take`: total[3] = the sizes of the vertex, chunk and body spaces
extern "C" void fs_totals(const int32_t* hulls, int nhulls, uint32_t take, int* total) {
    FleetTable t{};
    fleet_table(hulls, nhulls, take, &t);
    for (int s = 0; s < 3; s++) total[s] = t.total[s];
}

// fleet_map of every work index of `space` -> out [total][4] = hull, body within the hull, item, the body's index in the per-body arrays
extern "C" void fs_map_all(const int32_t* hulls, int nhulls, uint32_t take, int space, int* out) {
    FleetTable t{};
    fleet_table(hulls, nhulls, take, &t);
    for (int w = 0; w < t.total[space]; w++) {
        const FleetItem it = fleet_map(t, space, w);
        out[4 * w] = it.hull; out[4 * w + 1] = it.body; out[4 * w + 2] = it.item; out[4 * w + 3] = it.row.body_first + it.body;
    }
}

// fleet_integrate over n bodies [n][16] in place under rows [n][8], mass rows [n][8] and wrench rows [n][8] (or NULL); ok[n] = what it
// returned
extern "C" void fs_integrate(float* bodies, const float* rows, const float* mass, const float* wrench, int n, float g, float h, int* ok) {
    for (int b = 0; b < n; b++)
        ok[b] = fleet_integrate(bodies + 16 * b, rows + 8 * b, mass + 8 * b, wrench ? wrench + 8 * b : nullptr, g, h) ? 1 : 0;
}

// body_integrate, for the bit comparison with no wrench
extern "C" void fs_body_integrate(float* bodies, const float* rows, const float* mass, int n, float g, float h, int* ok) {
    for (int b = 0; b < n; b++) ok[b] = body_integrate(bodies + 16 * b, rows + 8 * b, mass + 8 * b, g, h) ? 1 : 0;
}

// fleet_wrench_valid of n wrench rows [n][8] -> ok[n]
extern "C" void fs_wrench_valid(const float* wrench, int n, int* ok) {
    for (int b = 0; b < n; b++) ok[b] = fleet_wrench_valid(wrench + 8 * b) ? 1 : 0;
}
