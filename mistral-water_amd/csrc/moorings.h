// moorings.h -- moorings: floating bodies tethered to fixed anchors by lines (mw_ocean_step_moored, include/mistral_water.h).
//
// A call carries K = lines_per_body slots per body, 1 <= K <= MW_MOORING_LINES, in lines [nbodies][K][MW_MOORING_SLOT]; one slot is
// three float4:   hx hy hz L0 | ax ay az k | c _ _ _
//   h   the attachment point in body space, about p, like the hull        L0  the unstretched length, >= 0
//   a   the anchor in the bodies' object space (world)                     k   the stiffness, >= 0        c  the damping along the line, >= 0
// A slot with k == 0 and c == 0 is empty and is skipped.  Per substep, at the state at its start (the state the water row is evaluated
// at), every non-empty slot in slot order:
//   1. d = R(q) h (hull_rotation, the R of the hull vertices), x = p + d.  d is the arm x - p, taken before p is added so that it
//      does not lose bits to |p|
//   2. va = v + w x d
//   3. r = a - x,  l = |r| = sqrt(rx rx + ry ry + rz rz)
//   4. l <= L0: the line is slack and contributes nothing (l == 0 included: nothing divides by zero)
//   5. e = r / l,  T = k (l - L0) - c (va . e), clamped below at 0: a line pulls and never pushes
//   6. F = T e,  tau = d x F
// The mooring wrench M = (F _ tau _) is the sum of the taut slots' (F, tau) in slot order, starting from the first taut slot's own
// value, not from zero.  With at least one slot taut, steps 2 and 3 of the integrator (rigid_bodies.h) see F[k] + M[k] and
// tau[k] + M[4 + k], one float32 add each -- fleet_pushed_row (rigid_bodies.h) with M as the wrench.  With no slot taut the water row is used as
// it is, no addition (adding a zero would turn a -0 into +0): the substep is body_integrate on the bare row.
// A slot is invalid when one of its nine used floats is not finite or L0, k or c is negative; the three padding floats are not read.
// One invalid slot makes the body's call invalid, like an invalid mass row.
//
// Stability: the integrator is the semi-implicit Euler of rigid_bodies.h; it needs h sqrt(k_total / m) < 2 for the stiffest direction
// (k_total the summed stiffness of the lines pulling along it).  Nothing here checks that.
//
// Strict float32: every function below sets its own `fp contract(off)`, so its multiplies and adds keep their own rounding in whichever
// translation unit it is inlined into, and the bits are those of tests/moorings_shim.cpp (g++ -ffp-contract=off).  The kernels that run them stand
// in surface_tiled.hip, which compiles the functions they share with the hull family (hull_rotation, body_integrate) strictly as well.
//
// Two plans with the same bits (surface_services.inc: moored_launch):
//   per substep   hull_launch's kernels, then k_moored_integrate (one lane per body: the slots as float4, the wrench, the pushed row,
//                 body_integrate), once per substep.  k_rigged_integrate (rigging.h) without targets computes the same bits and was
//                 measured in its place: 3.5-6 % slower per call, the target's four 16-byte loads per slot
//   one launch    k_fleet_step (fleet.h) on a one-hull table, with the body's slots staged once in LDS and lane 0 computing the
//                 wrench beside the integration (moored_integrate).  Strict kernels can share the substep loop; the one kernel
//                 that cannot is the contracted k_bodies_step<SqMesh> (rigid_bodies.h).
//
// Everything but the __global__ wrapper is MW_HD: tests/moorings_shim.cpp compiles the same functions with g++.
#pragma once
#include "rigid_bodies.h"  // fleet_integrate: the pushed row

namespace mw {

#define MW_MOORING_LINES 8   // slots per body at most (MW_MOORING_MAX_LINES)
#define MW_MOORING_SLOT 12   // floats per slot (MW_MOORING_NLINE)

#if defined(__clang__)
#define MW_MOORING_STRICT _Pragma("clang fp contract(off)")
#else
#define MW_MOORING_STRICT
#endif

// a usable slot: the nine used floats finite, L0, k and c not negative
MW_HD bool mooring_slot_valid(const float s[MW_MOORING_SLOT]) {
    for (int k = 0; k < 9; k++)
        if (!(fabsf(s[k]) <= 3.4e38f)) return false;
    return s[3] >= 0.f && s[7] >= 0.f && s[8] >= 0.f;
}

// Steps 1-6 of one slot for the body (p _ q v _ w _) with R = hull_rotation(q).  Returns true when the line is taut, with its pull in
// F and its torque about p in tau; *T is the tension, 0 for an empty or slack slot (F and tau then hold nothing of use).  Written
// without branches -- every step is computed and the answer selected -- so that lane 0 of k_fleet_step carries no nest of saved
// execution masks through its slot loop; a slack line's r / l may divide by zero, and its quotient is dropped unread.
MW_HD bool mooring_slot(const float body[16], const float R[9], const float s[MW_MOORING_SLOT], float F[3], float tau[3], float* T) {
    MW_MOORING_STRICT
    float d[3], r[3], va[3];
    for (int c = 0; c < 3; c++) d[c] = R[3 * c] * s[0] + R[3 * c + 1] * s[1] + R[3 * c + 2] * s[2];
    for (int c = 0; c < 3; c++) r[c] = s[4 + c] - (body[c] + d[c]);
    const float l = sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    const bool empty = s[7] == 0.f && s[8] == 0.f;
    const bool taut = !empty && l > s[3];  // l <= L0 is slack, l == 0 included
    const float* w = body + 12;
    va[0] = body[8] + (w[1] * d[2] - w[2] * d[1]);
    va[1] = body[9] + (w[2] * d[0] - w[0] * d[2]);
    va[2] = body[10] + (w[0] * d[1] - w[1] * d[0]);
    const float e[3] = {r[0] / l, r[1] / l, r[2] / l};
    float t = s[7] * (l - s[3]) - s[8] * (va[0] * e[0] + va[1] * e[1] + va[2] * e[2]);
    t = t < 0.f ? 0.f : t;
    *T = taut ? t : 0.f;
    for (int c = 0; c < 3; c++) F[c] = t * e[c];
    tau[0] = d[1] * F[2] - d[2] * F[1];
    tau[1] = d[2] * F[0] - d[0] * F[2];
    tau[2] = d[0] * F[1] - d[1] * F[0];
    return taut;
}

// The running sum of a body's taut slots, in the order they are added: M = (F _ tau _), floats 3 and 7 stay 0.
struct MooringSum {
    float M[8];
    bool any;    // a slot was taut: M holds a sum
    bool valid;  // every slot so far was valid
};
MW_HD void mooring_begin(MooringSum* m) {
    for (int k = 0; k < 8; k++) m->M[k] = 0.f;
    m->any = false;
    m->valid = true;
}
// takes one evaluated slot into the sum: a taut slot's (F, tau) is added (the first one is copied), any other leaves the sum as it is
MW_HD void mooring_take(MooringSum* m, bool taut, const float F[3], const float tau[3]) {
    MW_MOORING_STRICT
    for (int c = 0; c < 3; c++) {
        const float f = m->any ? m->M[c] + F[c] : F[c], q = m->any ? m->M[4 + c] + tau[c] : tau[c];
        m->M[c] = taut ? f : m->M[c];
        m->M[4 + c] = taut ? q : m->M[4 + c];
    }
    m->any = m->any || taut;
}
// adds one slot; returns its tension (an invalid slot's arithmetic passes through: the caller drops the sum when !valid)
MW_HD float mooring_add(MooringSum* m, const float body[16], const float R[9], const float s[MW_MOORING_SLOT]) {
    float F[3], tau[3], T;
    m->valid = m->valid && mooring_slot_valid(s);
    const bool taut = mooring_slot(body, R, s, F, tau, &T);
    mooring_take(m, taut, F, tau);
    return T;
}

// The mooring wrench of a body under its K slots lines [K][MW_MOORING_SLOT] -> M[8]; tension [K] (or nullptr) receives every slot's T.
// Returns -1 when a slot is invalid (M and tension are then NaN), 0 when no slot is taut (M is 0 and must not be added), 1 otherwise.
MW_HD int mooring_wrench(const float body[16], const float* lines, int K, float M[8], float* tension) {
    float R[9];
    hull_rotation(body + 4, R);
    MooringSum m;
    mooring_begin(&m);
    for (int s = 0; s < K; s++) {
        const float T = mooring_add(&m, body, R, lines + MW_MOORING_SLOT * s);
        if (tension) tension[s] = T;
    }
    if (!m.valid) {
        for (int k = 0; k < 8; k++) M[k] = NAN;
        if (tension)
            for (int s = 0; s < K; s++) tension[s] = NAN;
        return -1;
    }
    for (int k = 0; k < 8; k++) M[k] = m.M[k];
    return m.any ? 1 : 0;
}

// One substep of a moored body under its water row: the mooring wrench of the current state, the pushed row, body_integrate.  The slots
// must be valid (mooring_slot_valid).  Returns what body_integrate returns; a substep that leaves the body as it was (a NaN row) reports
// NaN tensions beside its NaN row, as an invalid slot does: a pose that is not known says nothing about its lines.
MW_HD bool moored_integrate(float body[16], const float row[8], const float mass[8], const float* lines, int K, float g, float h,
                            float* tension) {
    float M[8];
    const int taut = mooring_wrench(body, lines, K, M, tension);
    const bool ok = fleet_integrate(body, row, mass, taut > 0 ? M : nullptr, g, h);
    if (!ok && tension)
        for (int s = 0; s < K; s++) tension[s] = NAN;
    return ok;
}

// LDS k_fleet_step holds for a call's lines beyond k_bodies_step's: the staged slots and their tensions.  moored_one_launch
// (surface_services.inc) counts it as the plan rule of the moored call.
#define MW_MOORED_LDS_STATIC ((MW_MOORING_LINES * MW_MOORING_SLOT + MW_MOORING_LINES) * sizeof(float))

#if defined(__HIPCC__)
struct MooredArgs {
    float4* bodies;       // [nbodies][4] float4, updated in place
    const float4* mass;   // [nbodies][2]
    const float4* rows;   // hull_launch's rows of this substep [nbodies][2]
    const float4* lines;  // [nbodies][K][3]
    float4* out;          // [nbodies][2] or nullptr: the water row of the last substep
    float* tension;       // [nbodies][K] or nullptr: every slot's T at the start of the last substep
    float g, dt;          // gravity, h = dt / substeps
    int nbodies, K;
    int last;             // this is the call's last substep (write out and tension)
};

#if defined(MW_STRICT_LINE_KERNELS)  // one translation unit holds the line kernels (surface_tiled.hip): k_moored_integrate is no template
// Per-substep plan, after hull_launch: one lane per body.  The slots come in as three 16-byte loads each and are summed as they come,
// so no slot array is indexed at run time.
__global__ __launch_bounds__(256) void k_moored_integrate(MooredArgs a) {
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.nbodies) return;
    float body[16], mass[8], row[8], R[9];
    hull_load_body(a.bodies + 4 * b, body);
    hull_load_row(a.mass + 2 * b, mass);
    hull_load_row(a.rows + 2 * b, row);
    hull_rotation(body + 4, R);
    const bool tell = a.last && a.tension;
    MooringSum m;
    mooring_begin(&m);
    for (int s = 0; s < a.K; s++) {
        const float4* p = a.lines + 3 * ((size_t)b * a.K + s);
        const float4 s0 = p[0], s1 = p[1], s2 = p[2];
        const float slot[MW_MOORING_SLOT] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w, s2.x, s2.y, s2.z, s2.w};
        const float T = mooring_add(&m, body, R, slot);
        if (tell) a.tension[(size_t)b * a.K + s] = T;
    }
    if (!body_mass_valid(mass) || !m.valid) {
        for (int k = 0; k < 8; k++) row[k] = NAN;
        if (tell)
            for (int s = 0; s < a.K; s++) a.tension[(size_t)b * a.K + s] = NAN;
    } else if (fleet_integrate(body, row, mass, m.any ? m.M : nullptr, a.g, a.dt)) {
        for (int k = 0; k < 4; k++) a.bodies[4 * b + k] = make_float4(body[4 * k], body[4 * k + 1], body[4 * k + 2], body[4 * k + 3]);
    } else if (tell) {  // a NaN row: the body stays and its tensions are NaN (moored_integrate)
        for (int s = 0; s < a.K; s++) a.tension[(size_t)b * a.K + s] = NAN;
    }
    if (a.last && a.out) hull_store_row(a.out + 2 * b, row);
}
#endif  // MW_STRICT_LINE_KERNELS
#endif

}  // namespace mw
