// tests/rig_shim.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The MW_HD functions of the rigged fleets (mistral-water_amd/csrc/rigging.h) compiled with g++ for the CPU tier
// (tests/test_rigging_cpu.py) and as the bit reference of the GPU tier (tests/test_rigging_gpu.py): the line wrench of every body of
// an array and one substep over the whole array with snapshot semantics, on host arrays.  Never part of libmistral_water.so and not a
// fallback.
//
// build: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared (tests/shim_build.py)
#include <cstdint>
#include <vector>

#include "../mistral-water_amd/csrc/rigging.h"

using namespace mw;

// rig_wrench of every body of bodies [n][16] under lines [n][K][12] and targets [n][K] (or NULL) -> M [n][8], tension [n][K] (or NULL),
// state [n] = MW_RIG_INVALID -1, MW_RIG_NONE 0, MW_RIG_TAUT 1, MW_RIG_LOST 2
extern "C" void rs_wrench(const float* bodies, const float* lines, const int32_t* targets, int K, int n, float* M, float* tension,
                          int* state) {
    for (int b = 0; b < n; b++)
        state[b] = rig_wrench(bodies, n, b, lines + (size_t)MW_MOORING_SLOT * K * b, targets ? targets + (size_t)K * b : nullptr, K, M + 8 * b,
                              tension ? tension + (size_t)K * b : nullptr);
}

// One rigged substep of n bodies in place under the water rows [n][8], as k_rigged_integrate takes it: every body reads the copy of
// the array made before any body moved.  wrench [n][8] or NULL, g [n] the gravity of each body's hull, tension [n][K] or NULL.
// state [n]: -1 an invalid mass, wrench or slot row or a bad target (held, tension NaN), otherwise rigged_integrate's code
// (MW_RIG_LOST: held, tension NaN).
extern "C" void rs_step(float* bodies, const float* rows, const float* mass, const float* wrench, const float* lines,
                        const int32_t* targets, int K, int n, const float* g, float h, float* tension, int* state) {
    const std::vector<float> snap(bodies, bodies + 16 * (size_t)n);
    for (int b = 0; b < n; b++) {
        float* tn = tension ? tension + (size_t)K * b : nullptr;
        const float* wr = wrench ? wrench + 8 * b : nullptr;
        if (!body_mass_valid(mass + 8 * b) || (wr && !fleet_wrench_valid(wr))) {
            if (tn)
                for (int s = 0; s < K; s++) tn[s] = NAN;
            state[b] = MW_RIG_INVALID;
            continue;
        }
        state[b] = rigged_integrate(snap.data(), n, b, bodies + 16 * b, rows + 8 * b, mass + 8 * b, wr, lines + (size_t)MW_MOORING_SLOT * K * b,
                                    targets ? targets + (size_t)K * b : nullptr, K, g[b], h, tn);
    }
}
