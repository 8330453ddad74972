// tests/bodies_shim.cpp -- TEST INFRASTRUCTURE ONLY.
//
// The MW_HD functions of the floating-bodies feature (mistral-water_amd/csrc/rigid_bodies.h) compiled with g++ for the CPU tier
// (tests/test_bodies_cpu.py): the substep's integration and the mass-row check, on host arrays.  Never part of libmistral_water.so and
// not a fallback.
//
// build: g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared (tests/test_bodies_cpu.py)
#include <cstdint>

#include "../mistral-water_amd/csrc/rigid_bodies.h"

using namespace mw;

// body_integrate over n bodies [n][16] in place under rows [n][8] and mass rows [n][8]; ok[n] = what it returned
extern "C" void bs_integrate(float* bodies, const float* rows, const float* mass, int n, float g, float h, int* ok) {
    for (int b = 0; b < n; b++) ok[b] = body_integrate(bodies + 16 * b, rows + 8 * b, mass + 8 * b, g, h) ? 1 : 0;
}

// body_mass_valid of n mass rows [n][8] -> ok[n]
extern "C" void bs_mass_valid(const float* mass, int n, int* ok) {
    for (int b = 0; b < n; b++) ok[b] = body_mass_valid(mass + 8 * b) ? 1 : 0;
}
