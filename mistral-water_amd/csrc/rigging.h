// rigging.h -- rigged fleets: mooring lines and tow lines on a mixed fleet (mw_ocean_step_rigged, include/mistral_water.h).
//
// The call is mw_ocean_step_fleet (fleet.h) with moorings.h' slots, lines [total_bodies][K][MW_MOORING_SLOT], and one target per slot,
// targets [total_bodies][K] (nullptr: every slot is anchored):
//   MW_RIG_ANCHOR (-1)   the slot's a is a fixed world point: the slot is mooring_slot, bit for bit
//   j >= 0               a tow slot: a is an attachment point in the body space of body j of the call's bodies array
// Per substep every slot is evaluated at the SNAPSHOT, the state all bodies had at the start of that substep.  A tow slot of body i:
//   1. d = R(q_i) h, x = p_i + d, va = v_i + w_i x d           (mooring_slot's steps 1 and 2)
//   1'. dj = R(q_j) a, xj = p_j + dj, vb = v_j + w_j x dj       the same expressions on the target's state (rig_arm serves both ends)
//   3. r = xj - x, l = |r|        4. l <= L0: slack        5. e = r / l, T = k (l - L0) - c ((va - vb) . e), clamped below at 0
//   6. F = T e, tau = d x F
// Mirrored slots -- body i holds (h_i; a = h_j; target j) and body j holds (h_j; a = h_i; target i) with the same L0, k, c -- compute
// d and dj with their roles exchanged from the same expressions, so r and va - vb are exact negations, l, the dot product and T are equal
// bits and F_i == -F_j bitwise.  Nothing checks that a slot is mirrored: a one-sided slot pulls its owner alone.
//
// The body's line wrench M is the slot-order sum of its taut slots (MooringSum).  The integrator sees (F + W) + M: fleet_pushed_row with
// the external wrench W when the call has one, then fleet_pushed_row with M when a slot is taut; an absent part is no add.
// A body is invalid for the call (NaN out row, NaN tensions, state kept) when a slot is invalid (mooring_slot_valid) or a non-empty
// slot's target lies outside [-1, total_bodies) or is the body itself; an empty slot's target is not read.  A tow slot whose target's
// snapshot holds a non-finite float among p, q, v, w makes the owner's substep a NaN-row substep (state kept, NaN out row and tensions).
//
// One plan, per substep: fleet_rows' kernels, then k_rigged_integrate, one lane per body of the whole fleet, which reads the snapshot
// from one array and writes every body's next state to another (surface_services.inc: rig_launch ping-pongs the caller's array and a
// buffer of the handle), so that no lane reads a row a lane of the same launch writes.  DESIGN.md section 7m.
//
// Strict float32 as moorings.h: every function sets its own `fp contract(off)`, the kernel stands in surface_tiled.hip, and the bits
// are those of tests/rig_shim.cpp (g++ -ffp-contract=off).  Everything but the __global__ wrapper is MW_HD.
#pragma once
#include "fleet.h"  // the hull table; moorings.h: the slots

namespace mw {

#define MW_RIG_TARGET_ANCHOR (-1)  // MW_RIG_ANCHOR of the ABI

// what a slot's target asks of the evaluation
#define MW_RIG_SLOT_BAD (-1)  // a non-empty slot whose target is out of range or the owner itself
#define MW_RIG_SLOT_OWN 0     // empty or anchored: no other body is read (mooring_slot)
#define MW_RIG_SLOT_TOW 1     // reads body `target` of the snapshot
MW_HD int rig_slot_kind(const float s[MW_MOORING_SLOT], int target, int owner, int nbodies) {
    const bool empty = s[7] == 0.f && s[8] == 0.f;
    if (empty || target == MW_RIG_TARGET_ANCHOR) return MW_RIG_SLOT_OWN;
    return target >= 0 && target < nbodies && target != owner ? MW_RIG_SLOT_TOW : MW_RIG_SLOT_BAD;
}

// the thirteen floats of a state that a tow slot reads are finite (p q v w; floats 3, 11 and 15 are padding)
MW_HD bool rig_state_finite(const float body[16]) {
    bool ok = true;
    for (int k = 0; k < 15; k++) ok = ok && (k == 3 || k == 11 || fabsf(body[k]) <= 3.4e38f);
    return ok;
}

// One end of a line: the arm d = R h of the attachment point h about p and the velocity of that point, u = v + w x d -- mooring_slot's
// steps 1 and 2, expression for expression, for the owner and for the target alike.
MW_HD void rig_arm(const float body[16], const float R[9], const float h[3], float d[3], float u[3]) {
    MW_MOORING_STRICT
    for (int c = 0; c < 3; c++) d[c] = R[3 * c] * h[0] + R[3 * c + 1] * h[1] + R[3 * c + 2] * h[2];
    const float* w = body + 12;
    u[0] = body[8] + (w[1] * d[2] - w[2] * d[1]);
    u[1] = body[9] + (w[2] * d[0] - w[0] * d[2]);
    u[2] = body[10] + (w[0] * d[1] - w[1] * d[0]);
}

// A tow slot of `body` (R its rotation) to the attachment point s[4..6] of `other`, both at the snapshot: mooring_slot with the anchor
// replaced by the target's point and the closing speed (va - vb) . e.  Branch-free as mooring_slot is; returns true when taut.
MW_HD bool rig_tow_slot(const float body[16], const float R[9], const float s[MW_MOORING_SLOT], const float other[16], float F[3],
                        float tau[3], float* T) {
    MW_MOORING_STRICT
    float Rj[9], d[3], dj[3], va[3], vb[3], r[3], u[3];
    hull_rotation(other + 4, Rj);
    rig_arm(body, R, s, d, va);
    rig_arm(other, Rj, s + 4, dj, vb);
    for (int c = 0; c < 3; c++) r[c] = (other[c] + dj[c]) - (body[c] + d[c]);
    for (int c = 0; c < 3; c++) u[c] = va[c] - vb[c];
    const float l = sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
    const bool empty = s[7] == 0.f && s[8] == 0.f;
    const bool taut = !empty && l > s[3];
    const float e[3] = {r[0] / l, r[1] / l, r[2] / l};
    float t = s[7] * (l - s[3]) - s[8] * (u[0] * e[0] + u[1] * e[1] + u[2] * e[2]);
    t = t < 0.f ? 0.f : t;
    *T = taut ? t : 0.f;
    for (int c = 0; c < 3; c++) F[c] = t * e[c];
    tau[0] = d[1] * F[2] - d[2] * F[1];
    tau[1] = d[2] * F[0] - d[0] * F[2];
    tau[2] = d[0] * F[1] - d[1] * F[0];
    return taut;
}

// The running line wrench of a body: MooringSum and the two things only a rigged slot can do
struct RigSum {
    MooringSum m;
    bool bad;   // a target out of range or the owner's own index
    bool lost;  // a tow slot's target is not finite at the snapshot
};
MW_HD void rig_begin(RigSum* r) {
    mooring_begin(&r->m);
    r->bad = false;
    r->lost = false;
}
// adds one slot of kind `kind` (rig_slot_kind); other: the target's snapshot state, read only for MW_RIG_SLOT_TOW.  Returns the tension.
MW_HD float rig_add(RigSum* r, const float body[16], const float R[9], const float s[MW_MOORING_SLOT], int kind, const float other[16]) {
    if (kind != MW_RIG_SLOT_TOW) {
        r->bad = r->bad || kind == MW_RIG_SLOT_BAD;
        return mooring_add(&r->m, body, R, s);
    }
    float F[3], tau[3], T;
    r->m.valid = r->m.valid && mooring_slot_valid(s);
    r->lost = r->lost || !rig_state_finite(other);
    const bool taut = rig_tow_slot(body, R, s, other, F, tau, &T);
    mooring_take(&r->m, taut, F, tau);
    return T;
}

// what rig_wrench and rigged_integrate report
#define MW_RIG_INVALID (-1)  // the body is invalid for the call: M and the tensions are NaN
#define MW_RIG_NONE 0        // no slot taut: M is 0 and must not be added
#define MW_RIG_TAUT 1        // M holds the sum
#define MW_RIG_LOST 2        // a target is not finite: a NaN-row substep, M and the tensions are NaN

// The line wrench of body b of the snapshot snap [nbodies][16] under its K slots lines [K][MW_MOORING_SLOT] and targets [K] (nullptr:
// all anchored) -> M[8]; tension [K] (or nullptr) receives every slot's T.
MW_HD int rig_wrench(const float* snap, int nbodies, int b, const float* lines, const int32_t* targets, int K, float M[8], float* tension) {
    const float* body = snap + 16 * (size_t)b;
    float R[9];
    hull_rotation(body + 4, R);
    RigSum r;
    rig_begin(&r);
    for (int s = 0; s < K; s++) {
        const float* slot = lines + MW_MOORING_SLOT * s;
        const int t = targets ? targets[s] : MW_RIG_TARGET_ANCHOR;
        const int kind = rig_slot_kind(slot, t, b, nbodies);
        const float T = rig_add(&r, body, R, slot, kind, snap + 16 * (size_t)(kind == MW_RIG_SLOT_TOW ? t : b));
        if (tension) tension[s] = T;
    }
    const bool valid = r.m.valid && !r.bad;
    if (!valid || r.lost) {
        for (int k = 0; k < 8; k++) M[k] = NAN;
        if (tension)
            for (int s = 0; s < K; s++) tension[s] = NAN;
        return valid ? MW_RIG_LOST : MW_RIG_INVALID;
    }
    for (int k = 0; k < 8; k++) M[k] = r.m.M[k];
    return r.m.any ? MW_RIG_TAUT : MW_RIG_NONE;
}

// The end of a rigged substep once the line wrench is known: `state` (MW_RIG_NONE or MW_RIG_TAUT with M) -> the row (F + W) + M and
// body_integrate on it.  wrench: the body's external wrench row or nullptr.  Returns what body_integrate returns.
MW_HD bool rig_push(float body[16], const float row[8], const float mass[8], const float* wrench, int state, const float M[8], float g,
                    float h) {
    float pushed[8];
    fleet_pushed_row(row, wrench, pushed);
    return fleet_integrate(body, pushed, mass, state == MW_RIG_TAUT ? M : nullptr, g, h);
}

// One substep of body b: its line wrench at the snapshot, the pushed row, body_integrate into next[16] (the snapshot state when the
// body is held).  The mass and wrench rows must be valid.  Returns rig_wrench's code, or MW_RIG_LOST as well when the water row is NaN
// (the tensions are then NaN, as moored_integrate's).
MW_HD int rigged_integrate(const float* snap, int nbodies, int b, float next[16], const float row[8], const float mass[8],
                           const float* wrench, const float* lines, const int32_t* targets, int K, float g, float h, float* tension) {
    float M[8];
    for (int k = 0; k < 16; k++) next[k] = snap[16 * (size_t)b + k];
    const int state = rig_wrench(snap, nbodies, b, lines, targets, K, M, tension);
    if (state == MW_RIG_INVALID || state == MW_RIG_LOST) return state;
    if (rig_push(next, row, mass, wrench, state, M, g, h)) return state;
    if (tension)
        for (int s = 0; s < K; s++) tension[s] = NAN;
    return MW_RIG_LOST;
}

#if defined(__HIPCC__)
struct RigArgs {
    const float4* snap;      // [total_bodies][4] float4: the state at the start of the substep
    float4* next;            // [total_bodies][4] float4: every body's state after it (another array than snap)
    const float4* mass;      // [total_bodies][2]
    const float4* wrench;    // [total_bodies][2] or nullptr
    const float4* rows;      // fleet_rows' rows of this substep [total_bodies][2]
    const float4* lines;     // [total_bodies][K][3]
    const int32_t* targets;  // [total_bodies][K] or nullptr
    float4* out;             // [total_bodies][2] or nullptr: the water row of the last substep
    float* tension;          // [total_bodies][K] or nullptr: every slot's T at the start of the last substep
    float dt;                // h = dt / substeps
    int K;
    int last;                // this is the call's last substep (write out and tension)
    FleetTable t;            // every hull of the call: total[MW_FLEET_BODIES] == total_bodies
};

#if defined(MW_STRICT_LINE_KERNELS)
// One lane per body of the whole fleet.  The slots come in as three 16-byte loads each, a tow slot's target as four, and are summed as
// they come.  Reads bodies from snap only and writes them to next only.
__global__ __launch_bounds__(256) void k_rigged_integrate(RigArgs a) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int n = a.t.total[MW_FLEET_BODIES];
    if (w >= n) return;
    const FleetItem it = fleet_map(a.t, MW_FLEET_BODIES, (int)w);
    const int b = it.row.body_first + it.body;
    float body[16], mass[8], row[8], wr[8], R[9];
    float4 keep[4];
    for (int k = 0; k < 4; k++) keep[k] = a.snap[4 * (size_t)b + k];
    hull_load_body(keep, body);
    hull_load_row(a.mass + 2 * (size_t)b, mass);
    hull_load_row(a.rows + 2 * (size_t)b, row);
    bool valid = body_mass_valid(mass);
    if (a.wrench) {
        hull_load_row(a.wrench + 2 * (size_t)b, wr);
        valid = valid && fleet_wrench_valid(wr);
    }
    hull_rotation(body + 4, R);
    const bool tell = a.last && a.tension;
    RigSum r;
    rig_begin(&r);
    for (int s = 0; s < a.K; s++) {
        const size_t k = (size_t)b * a.K + s;
        const float4* p = a.lines + 3 * k;
        const float4 s0 = p[0], s1 = p[1], s2 = p[2];
        const float slot[MW_MOORING_SLOT] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w, s2.x, s2.y, s2.z, s2.w};
        const int t = a.targets ? a.targets[k] : MW_RIG_TARGET_ANCHOR;
        const int kind = rig_slot_kind(slot, t, b, n);
        float other[16];
        hull_load_body(a.snap + 4 * (size_t)(kind == MW_RIG_SLOT_TOW ? t : b), other);  // in range whatever t holds
        const float T = rig_add(&r, body, R, slot, kind, other);
        if (tell) a.tension[k] = T;
    }
    bool moved = false;
    if (!valid || !r.m.valid || r.bad || r.lost) {
        for (int k = 0; k < 8; k++) row[k] = NAN;
    } else {
        moved = rig_push(body, row, mass, a.wrench ? wr : nullptr, r.m.any ? MW_RIG_TAUT : MW_RIG_NONE, r.m.M, it.row.g, a.dt);
    }
    if (!moved && tell)  // held: invalid, a lost target or a NaN row
        for (int s = 0; s < a.K; s++) a.tension[(size_t)b * a.K + s] = NAN;
    for (int k = 0; k < 4; k++)
        a.next[4 * (size_t)b + k] = moved ? make_float4(body[4 * k], body[4 * k + 1], body[4 * k + 2], body[4 * k + 3]) : keep[k];
    if (a.last && a.out) hull_store_row(a.out + 2 * (size_t)b, row);
}
#endif  // MW_STRICT_LINE_KERNELS
#endif

}  // namespace mw
