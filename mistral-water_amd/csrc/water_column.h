// water_column.h -- the water below the surface: velocity and rest depth at points in the water column
// (mw_ocean_set_column / mw_ocean_query_column, include/mistral_water.h).
//
// A deep-water component of wave number k decays as e^{-k d} at rest depth d, and every output of a frame is linear in the spectrum: the
// water that rests at depth d_l is the frame pipeline's output on the attenuated spectrum (A_l h0, A_l h0c), A_l = e^{-k d_l}, and its
// velocity the velocity pipeline's on (i w A_l h0, -i w A_l h0c) (velocity_kernels.h).  A_l is real and a function of the float k whose
// sqrt(g k) is the dispersion, so it is mirror-symmetric bit for bit exactly as omega is and survives k_prep's pairing.  A column is L such
// layers, d_0 = 0 < d_1 < ... < d_{L-1}; layer 0 is the surface mesh and the surface velocity themselves.  Layer l is two [R*R][3] arrays:
// pos_l, the displaced vertices with y = h_l (the layer's height is h_l - d_l, subtracted once, after interpolation), and vel_l.
//
// In this Lagrangian first-order model the pressure on a material surface is rho g times its rest depth (exact for one trochoidal wave,
// first order for the sum), so the rest depth of the particle at a world point is the pressure there.
//
// A world query (x, y, z) scans the layers from the top: in layer l it locates (x, z) with the one sq_locate of the surface services on
// pos_l, which gives the layer's height y_l there, its velocity, the located rest point and a residual, and stops at the first l with
// y > y_{l+1}.  By induction y_{l+1} < y <= y_l, so s = (y_l - y) / (y_l - y_{l+1}) never divides by zero or a negative number.  Layers
// below l + 1 are not located; a point exactly on layer l (y == y_l) is that layer's sample and layer l + 1 is not located either, so a
// height fed back from the surface query gets the surface's own residual.  A rest query (x0, d, z0) names the particle by its label: the cell and the weights are the same in every
// layer, so it locates once.  Every blend between layers is (1 - s) a + s b in strict float32 (exact at s = 0 and s = 1), every gather
// inside a layer accumulates sum w_k value_k in corner order as sq_query_point and sq_velocity_point do.
//
// Everything but the __global__ wrappers is MW_HD: tests/column_shim.cpp compiles the same functions with g++ -ffp-contract=off, and the
// kernels are compiled without contraction too (water_column.hip), SqMesh instantiation included: device and shim agree bit for bit.
#pragma once
#include "surface_query.h"
#include "velocity_kernels.h"  // velocity_weight

namespace mw {

#define MW_COL_MAX_LAYERS 16
#define MW_COL_NOUT 12  // ux uy uz rest_depth | px py pz lambda | x0 z0 eta residual

// the layer table of a query: travels as a kernel argument (device pointers on the GPU, host pointers in the shim)
struct ColTable {
    int L;
    float depth[MW_COL_MAX_LAYERS];
    const float* pos[MW_COL_MAX_LAYERS];  // [R*R][3]; pos[0] is the surface mesh
    const float* vel[MW_COL_MAX_LAYERS];  // [R*R][3]; vel[0] is the surface velocity
};

// ---- the layer builder ----
// wave number of spectrum bin (n, m): the float whose sqrt(g k) omega_f32 floors, formed exactly as omega_f32 forms it
MW_HD float column_wave_number(int N, float length, int n, int m) {
    float kx = sdiv(smul(MW_PI_F, (float)(2 * n - N)), length);
    float kz = sdiv(smul(MW_PI_F, (float)(2 * m - N)), length);
    return ssqrt(sadd(smul(kx, kx), smul(kz, kz)));
}
MW_HD float column_attenuation(int N, float length, int n, int m, float depth) { return expf(-smul(column_wave_number(N, length, n, m), depth)); }
// (h0, h0c) -> the position pair (A h0, A h0c) and the velocity pair (i w A h0, -i w A h0c): attenuated first, then weighted
MW_HD void column_weight(float A, float w, cf a, cf b, cf* pa, cf* pb, cf* va, cf* vb) {
    *pa = mk(smul(A, a.x), smul(A, a.y));
    *pb = mk(smul(A, b.x), smul(A, b.y));
    velocity_weight(w, *pa, *pb, va, vb);
}

// ---- queries ----
MW_HD float col_mix(float s, float a, float b) { return sadd(smul(ssub(1.f, s), a), smul(s, b)); }

// one layer at a located point, in the frame of the locate (the base tile on a periodic handle): velocity, position with y = h - d, the
// rest point
struct ColPoint { float u[3], p[3], x0, z0; };

template <typename Mesh>
MW_HD void col_gather(const Mesh& m, const float* pos, const float* vel, float d, const int v[3], const float w[3], const SqTile& t, ColPoint* c) {
    Mesh ml = m;
    ml.vert = pos;
    float p[3] = {0.f, 0.f, 0.f}, u[3] = {0.f, 0.f, 0.f}, x0 = 0.f, z0 = 0.f;
    for (int k = 0; k < 3; k++) {
        const float x[3] = {sq_corner_x(ml, t, v[k], k), pos[3 * v[k] + 1], sq_corner_z(ml, t, v[k], k)};
        const int i = v[k] / m.R, j = v[k] - i * m.R;
        float rx = rest_coord(m.R, m.unit_width, i), rz = rest_coord(m.R, m.unit_width, j);
        if constexpr (Mesh::tiled) { rx = sq_shift(rx, t.ki[k], m.period); rz = sq_shift(rz, t.kj[k], m.period); }
        for (int c3 = 0; c3 < 3; c3++) {
            p[c3] += w[k] * x[c3];
            u[c3] += w[k] * vel[3 * v[k] + c3];
        }
        x0 += w[k] * rx;
        z0 += w[k] * rz;
    }
    for (int c3 = 0; c3 < 3; c3++) { c->p[c3] = p[c3]; c->u[c3] = u[c3]; }
    c->p[1] = p[1] - d;
    c->x0 = x0; c->z0 = z0;
}

// What a query resolves to before it is written out: the blended (or single) layer sample in the frame of the locate, the scalars of the
// row, the tile of the point.  One writer (col_row) turns it into the 12 floats, so that no path indexes the row dynamically.
struct ColAnswer { ColPoint a; float rest_depth, lambda, eta, residual; int kx, kz; bool ok; };
MW_HD ColPoint col_blend(float s, const ColPoint& a, const ColPoint& b) {
    ColPoint r;
    for (int c = 0; c < 3; c++) { r.u[c] = col_mix(s, a.u[c], b.u[c]); r.p[c] = col_mix(s, a.p[c], b.p[c]); }
    r.x0 = col_mix(s, a.x0, b.x0);
    r.z0 = col_mix(s, a.z0, b.z0);
    return r;
}
// out = ux uy uz rest_depth | px py pz lambda | x0 z0 eta residual; on the tiling the tile offset goes on px, pz, x0, z0 last
template <typename Mesh>
MW_HD void col_row(const Mesh& m, const ColAnswer& q, float out[MW_COL_NOUT]) {
    float px = q.a.p[0], pz = q.a.p[2], x0 = q.a.x0, z0 = q.a.z0;
    if constexpr (Mesh::tiled) {
        px = sq_shift(px, q.kx, m.period); pz = sq_shift(pz, q.kz, m.period);
        x0 = sq_shift(x0, q.kx, m.period); z0 = sq_shift(z0, q.kz, m.period);
    }
    const float row[MW_COL_NOUT] = {q.a.u[0], q.a.u[1], q.a.u[2], q.rest_depth, px, q.a.p[1], pz, q.lambda, x0, z0, q.eta, q.residual};
    for (int k = 0; k < MW_COL_NOUT; k++) out[k] = q.ok ? row[k] : NAN;
}

// MW_QUERY_WORLD: (x, y, z) is a position in the water.  The layer index of the loop is the same in every lane of a wave, so the table is
// read with uniform indices.
template <typename Mesh>
MW_HD void col_world_point(const Mesh& m, const ColTable& tb, float qx, float qy, float qz, int iters, ColAnswer* q) {
    q->ok = false;
    if (!(fabsf(qy) <= 3.4e38f)) return;
    ColPoint prev{}, cur{};
    for (int l = 0; l < tb.L; l++) {
        bool ok = false;
        float r = 0.f;
        Mesh ml = m;
        ml.vert = tb.pos[l];
        const float* vel = tb.vel[l];
        const float d = tb.depth[l];
        sq_locate(ml, MW_SQ_WORLD, qx, qz, iters, [] {}, [&](const int v[3], const float w[3], const SqTile& t) {
            ok = true;
            col_gather(m, ml.vert, vel, d, v, w, t, &cur);
            const float ex = cur.p[0] - t.qx, ez = cur.p[2] - t.qz;
            r = sqrtf(ex * ex + ez * ez);
            if constexpr (Mesh::tiled) { q->kx = t.kx; q->kz = t.kz; }
        });
        if (!ok) return;  // a layer whose locate has no answer: the row of NaN
        if (l == 0) {
            q->eta = cur.p[1]; q->residual = r;
            if (qy > cur.p[1]) {  // in the air: layer 0's point, no velocity, the (negative) height above the surface
                q->a = cur;
                q->a.u[0] = q->a.u[1] = q->a.u[2] = 0.f;
                q->rest_depth = cur.p[1] - qy; q->lambda = 0.f; q->ok = true;
                return;
            }
        } else {
            q->residual = fmaxf(q->residual, r);
            if (qy > cur.p[1]) {  // cur.p[1] < qy <= prev.p[1]
                const float s = (prev.p[1] - qy) / (prev.p[1] - cur.p[1]);
                q->a = col_blend(s, prev, cur);
                q->rest_depth = col_mix(s, tb.depth[l - 1], d); q->lambda = (float)(l - 1) + s; q->ok = true;
                return;
            }
        }
        if (qy == cur.p[1]) {  // exactly on layer l: its sample, s = 0; nothing deeper is located
            q->a = cur;
            q->rest_depth = d; q->lambda = (float)l; q->ok = true;
            return;
        }
        prev = cur;
    }
    // at or below the deepest layer: its point and velocity, the hydrostatic continuation of the rest depth
    q->a = prev;
    q->rest_depth = tb.depth[tb.L - 1] + (prev.p[1] - qy); q->lambda = (float)(tb.L - 1); q->ok = true;
}

// MW_QUERY_REST: (x0, d, z0) is a particle label; one rest-mode locate, the two layers around d gathered with its weights
template <typename Mesh>
MW_HD void col_rest_point(const Mesh& m, const ColTable& tb, float qx, float qd, float qz, ColAnswer* q) {
    q->ok = false;
    if (!(qd >= 0.f && qd <= tb.depth[tb.L - 1])) return;  // NaN ends here too
    Mesh m0 = m;
    m0.vert = tb.pos[0];
    sq_locate(m0, MW_SQ_REST, qx, qz, 0, [] {}, [&](const int v[3], const float w[3], const SqTile& t) {
        ColPoint a{}, b{};
        col_gather(m, tb.pos[0], tb.vel[0], 0.f, v, w, t, &a);
        q->eta = a.p[1];
        // the last layer with d_l <= d, capped at L - 2; the loop index, not l, reads the table (uniform in a wave)
        for (int k = 0; k + 1 < tb.L; k++) {
            const bool last = k + 2 == tb.L;
            if (!(qd >= tb.depth[k] && (last || qd < tb.depth[k + 1]))) continue;
            if (k > 0) col_gather(m, tb.pos[k], tb.vel[k], tb.depth[k], v, w, t, &a);
            col_gather(m, tb.pos[k + 1], tb.vel[k + 1], tb.depth[k + 1], v, w, t, &b);
            const float s = (qd - tb.depth[k]) / (tb.depth[k + 1] - tb.depth[k]);
            q->a = col_blend(s, a, b);
            q->rest_depth = qd; q->lambda = (float)k + s; q->residual = 0.f; q->ok = true;
            if constexpr (Mesh::tiled) { q->kx = t.kx; q->kz = t.kz; }
            break;
        }
    });
}

template <typename Mesh>
MW_HD void col_query_point(const Mesh& m, const ColTable& tb, int mode, float x, float y, float z, int iters, float out[MW_COL_NOUT]) {
    ColAnswer q{};
    if (mode == MW_SQ_REST) col_rest_point(m, tb, x, y, z, &q);
    else col_world_point(m, tb, x, y, z, iters, &q);
    col_row(m, q, out);
}

#if defined(__HIPCC__)
#if defined(MW_COL_KERNELS)  // water_column.hip: a kernel that is no template stands in one translation unit
// One lane per spectrum bin, one layer per launch: the attenuated pair and its velocity pair.
__global__ void k_column_weight(int N, float length, float gravity, float depth, const cf* __restrict__ h0, const cf* __restrict__ h0c,
                                cf* __restrict__ ph0, cf* __restrict__ ph0c, cf* __restrict__ vh0, cf* __restrict__ vh0c) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * N) return;
    const int n = idx / N, m = idx % N;
    column_weight(column_attenuation(N, length, n, m, depth), omega_f32(N, length, gravity, n, m), h0[idx], h0c[idx], &ph0[idx], &ph0c[idx],
                  &vh0[idx], &vh0c[idx]);
}
#endif
// One lane per point: a 16-byte load of (x, y, z, _), per layer visited the walk's dependent 3-vertex gathers and one gather of the
// layer's positions and velocities, three 16-byte stores.  No LDS, no atomics, no ordering between workgroups.
template <typename Mesh>
__global__ __launch_bounds__(256) void k_query_column(Mesh m, ColTable tb, int mode, int iters, const float4* __restrict__ xyz, int64_t n,
                                                      float4* __restrict__ out) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= n) return;
    const float4 q = xyz[k];
    float r[MW_COL_NOUT];
    col_query_point(m, tb, mode, q.x, q.y, q.z, iters, r);
    out[3 * k] = make_float4(r[0], r[1], r[2], r[3]);
    out[3 * k + 1] = make_float4(r[4], r[5], r[6], r[7]);
    out[3 * k + 2] = make_float4(r[8], r[9], r[10], r[11]);
}

// how the host code (surface_services.inc) launches the kernels of water_column.hip; each enqueues on s and returns hipGetLastError()
#ifndef MW_INTERNAL
#define MW_INTERNAL __attribute__((visibility("hidden")))
#endif
MW_INTERNAL hipError_t column_weight_launch(hipStream_t s, int N, float length, float gravity, float depth, const cf* h0, const cf* h0c, cf* ph0,
                                            cf* ph0c, cf* vh0, cf* vh0c);
// m.period != 0 selects the SqTiled instantiation
MW_INTERNAL hipError_t column_query_launch(hipStream_t s, const SqMesh& m, const ColTable& tb, int mode, int iters, const float4* xyz, int64_t n,
                                           float4* out);
#endif

}  // namespace mw
