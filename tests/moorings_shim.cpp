// tests/moorings_shim.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The MW_HD functions of the moorings (mistral-water_amd/csrc/moorings.h) and the integrator they push (rigid_bodies.h) compiled with
// g++ for the CPU tier (tests/test_moorings_cpu.py) and as the bit reference of the GPU tier (tests/test_moorings_gpu.py): the mooring
// wrench, one moored substep and the slot check, on host arrays.  Never part of libmistral_water.so and not a fallback.
//
// build: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared (tests/shim_build.py)
#include <cstdint>

#include "../mistral-water_amd/csrc/moorings.h"
#include "../mistral-water_amd/csrc/rigid_bodies.h"

using namespace mw;

// mooring_wrench of n bodies [n][16] under lines [n][K][12] -> M [n][8], tension [n][K] (or NULL), taut [n] = -1 invalid, 0 none, 1 some
extern "C" void ms_wrench(const float* bodies, const float* lines, int K, int n, float* M, float* tension, int* taut) {
    for (int b = 0; b < n; b++)
        taut[b] = mooring_wrench(bodies + 16 * b, lines + (size_t)MW_MOORING_SLOT * K * b, K, M + 8 * b, tension ? tension + (size_t)K * b : nullptr);
}

// One moored substep of n bodies in place under the water rows [n][8], as the kernels take it: an invalid mass row or slot leaves the
// body as it is (ok = -1, tension NaN), otherwise moored_integrate (ok = what it returned).  tension [n][K] or NULL.
extern "C" void ms_step(float* bodies, const float* rows, const float* mass, const float* lines, int K, int n, float g, float h,
                        float* tension, int* ok) {
    for (int b = 0; b < n; b++) {
        const float* ln = lines + (size_t)MW_MOORING_SLOT * K * b;
        float* tn = tension ? tension + (size_t)K * b : nullptr;
        bool valid = body_mass_valid(mass + 8 * b);
        for (int s = 0; s < K; s++) valid = valid && mooring_slot_valid(ln + MW_MOORING_SLOT * s);
        if (!valid) {
            if (tn)
                for (int s = 0; s < K; s++) tn[s] = NAN;
            ok[b] = -1;
            continue;
        }
        ok[b] = moored_integrate(bodies + 16 * b, rows + 8 * b, mass + 8 * b, ln, K, g, h, tn) ? 1 : 0;
    }
}

// body_integrate, for the bit comparison with every line slack
extern "C" void ms_body_integrate(float* bodies, const float* rows, const float* mass, int n, float g, float h, int* ok) {
    for (int b = 0; b < n; b++) ok[b] = body_integrate(bodies + 16 * b, rows + 8 * b, mass + 8 * b, g, h) ? 1 : 0;
}

// the LDS k_fleet_step holds for a call's lines beside the slab and partials: the plan rule of moored_one_launch (surface_services.inc)
extern "C" int64_t ms_moored_lds_static() { return (int64_t)MW_MOORED_LDS_STATIC; }

// mooring_slot_valid of n slots [n][12] -> ok[n]
extern "C" void ms_slot_valid(const float* slots, int n, int* ok) {
    for (int s = 0; s < n; s++) ok[s] = mooring_slot_valid(slots + MW_MOORING_SLOT * s) ? 1 : 0;
}
