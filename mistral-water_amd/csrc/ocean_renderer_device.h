// ocean_renderer_device.h -- __global__ wrappers and host-side state of MW_SEM_OCEANRENDERER (device build only).
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <utility>
#include <vector>

#include "../../include/mistral_water.h"
#include "mw_host.h"
#include "ocean_renderer_kernels.h"
#include "mw_switches.h"

namespace mw {

// One set of the seven arrays a frame is made of.  The handle holds two: `out`, the latest frame (tile-major on a batched handle), and
// `fr`, the frame buffers of a steps call ([frames_cap] frames each).  A set whose height_g / disp_a are NULL is a planar frame.
struct OrTex {
    float* height = nullptr;  // heightTexture.r
    cf* disp = nullptr;       // displacementTexture.rb: (x, z) pairs
    float *disp_g = nullptr, *normal = nullptr, *white = nullptr;
    float *height_g = nullptr, *disp_a = nullptr;  // Im h, Im Dz: written only by the calls that deliver the RGBA layout
    // the set `texels` further on: frame k of the frame buffers is at(k * M * M)
    OrTex at(size_t texels) const {
        auto mv = [texels](auto* p, size_t per) { return p ? p + per * texels : p; };
        return OrTex{mv(height, 1), mv(disp, 1), mv(disp_g, 1), mv(normal, 3), mv(white, 1), mv(height_g, 1), mv(disp_a, 1)};
    }
    OrTex real_only() const { OrTex t = *this; t.height_g = t.disp_a = nullptr; return t; }
};
// `tiles` independent oceans (seed, seed + 1, ...) share one handle: every buffer below carries a leading tile axis and
// every kernel one more grid dimension, so a GenerateTexture() of all tiles is still three launches (mw_ocean_create_batch).
// A frame of ONE 1024^2 texture is latency-bound (three launches of 256-768 workgroups); the phase recurrence forbids
// batching in time, so the tile axis is what fills the machine.  omT (a function of k alone) is shared by the tiles.
struct OrState {
    int M = 0;
    int tiles = 1;
    OrConsts c{};  // c.choppiness: that of the latest frame (or_frames sets it; or_velocity differentiates that frame)
    float mult = 1.f;
    f4* initT = nullptr;
    f4* PQT = nullptr;     // [px][py] Hermitian parts (P, Q) of the initial spectrum: the packed plan (or_prep_element), rebuilt with initT
    bool phase_sym = true; // the phase texture equals its mirror image (true from creation on; mw_ocean_set_phase checks what it is given)
    float* omT = nullptr;  // [px][py] angular frequency (or_omega), fixed per handle
    float *phaseT = nullptr, *phaseT2 = nullptr;  // current phase / next phase (swapped after every frame)
    cf *TW = nullptr, *E = nullptr;
    OrTex out;  // the latest frame; height_g / disp_a allocated by the first call that asks for the RGBA layout (or_imag_planes)
    bool have_frame = false;
    // mw_ocean_generate_texture_steps_device: [frames_cap] frames of the exchange buffer and of the textures the caller did not ask for
    // (disp.g always: OceanNormal reads it, no entry point hands it out alone); grown on demand, never shrunk
    int frames_cap = 0, frames_last = 0;  // capacity / frames of the latest steps call
    cf* fr_E = nullptr;
    OrTex fr;
    bool fr_have[4] = {false, false, false, false};  // which textures the latest steps call kept here
};

__global__ void k_or_omega(OrConsts c, float* omT) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= c.M * c.M) return;
    omT[idx] = or_omega(c, idx / c.M, idx % c.M);  // transposed enumeration [px][py]
}
__global__ void k_or_init(int M, float length, float wind_x, float wind_y, float amp, float gravity, uint64_t seed, f4* initT,
                          float* phaseT) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * M) return;
    const size_t toff = (size_t)blockIdx.y * M * M;  // tile blockIdx.y: seed + tile
    // idx enumerates the transposed array (px major) so the writes coalesce
    or_init_element(M, length, wind_x, wind_y, amp, gravity, seed + blockIdx.y, idx / M, idx % M, initT + toff,
                    phaseT ? phaseT + toff : nullptr);
}

// initialTexture <-> (h0, h0conj) arrays in the reference's texel order idx = py*M + px
__global__ void k_or_set_init(int M, const cf* h0, const cf* h0c, f4* initT, float* phaseT) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * M) return;
    const size_t toff = (size_t)blockIdx.y * M * M;
    h0 += toff; h0c += toff; initT += toff; phaseT += toff;
    const int px = idx / M, py = idx % M;  // transposed enumeration: coalesced writes
    const cf a = h0[(size_t)py * M + px], b = h0c[(size_t)py * M + px];
    f4 v; v.x = a.x; v.y = a.y; v.z = b.x; v.w = b.y;
    initT[idx] = v;
    phaseT[idx] = 0.f;  // RenderInitial does not touch the phase in the reference; a fresh spectrum restarts it here
}
__global__ void k_or_get_init(int M, const f4* initT, cf* h0, cf* h0c) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * M) return;
    const size_t toff = (size_t)blockIdx.y * M * M;
    initT += toff; h0 += toff; h0c += toff;
    const int py = idx / M, px = idx % M;
    const f4 v = initT[(size_t)px * M + py];
    h0[idx] = mk(v.x, v.y);
    h0c[idx] = mk(v.z, v.w);
}

__global__ void k_or_prep(int M, const f4* initT, f4* PQT) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * M) return;
    const size_t toff = (size_t)blockIdx.y * M * M;  // tile blockIdx.y
    or_prep_element(M, idx / M, idx % M, initT + toff, PQT + toff);
}
#ifndef MW_OR_P1_LONE_CHUNK
#define MW_OR_P1_LONE_CHUNK 4  // points whose loads the lone frame's spectrum workgroup requests together (1 / 2 / 4 / 8: 1024^2 34.4 / 34.1 / 34.0 /
#endif                         // 34.7 us per frame, 512^2 19.9 / 19.0 / 18.9 / 18.9; the three-transform plan keeps point by point)
#ifndef MW_OR_PACKED_MAX_M
#define MW_OR_PACKED_MAX_M 4096  // textures from this size up keep the three-transform plan
#endif
#ifndef MW_OR_PACKED
#define MW_OR_PACKED 1  // planar-texture calls with a mirror-symmetric phase run two transforms per frame (0: always three)
#endif

// the packed plan's spectrum kernel (lone frame: gridDim.y == 2, one field per workgroup; tiles / big textures: gridDim.y == 1, both fields)
template <int N, int P>
__global__ __launch_bounds__((OrP1Geom<N, P>::NTHREADS)) void k_or_pass1_packed(OrP1Args A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using G = OrP1Geom<N, P>;
    cf* lds = reinterpret_cast<cf*>(smem);
    constexpr int T = FftGeom<N, P>::T;
    const int tid = threadIdx.x, jb = blockIdx.x;
    const int f0 = gridDim.y == 1 ? 0 : (int)blockIdx.y, f1 = gridDim.y == 1 ? 2 : f0 + 1;
    {   // tile blockIdx.z of a batched handle
        const size_t toff = (size_t)blockIdx.z * N * N;
        A.initT += toff; A.PQT += toff; A.phase_in += toff; A.phase_out += toff; A.E += 2 * toff;
    }
    const int w = tid / T, u = tid % T;
    TwStage<N, P, G::NTHREADS, false> tws;
    tws.load(A.TW, tid);
    const Twiddles tw = TwGeom<N, P>::view(A.TW, lds);
    cf* set0 = lds + G::TW_LDS;
    cf h[P], hh[P], x[P];
#pragma unroll
    for (int q = 0; q < P; q++) h[q] = hh[q] = mk(0.f, 0.f);
    if (gridDim.y == 1) or_p1_animate_packed<N, P, MW_OR_P1_CHUNK>(A, jb, tid, true, true, true, h, hh);
    else or_p1_animate_packed<N, P, MW_OR_P1_LONE_CHUNK>(A, jb, tid, f0 == 0, f0 == 0, f0 == 1, h, hh);
    tws.store(lds, tid);
    for (int f = f0; f < f1; f++) {
        or_p1_build_packed<N, P>(A, jb, tid, f, h, hh, x);
        if (f != f0) __syncthreads();
        stage0_store<N, P, -1>(x, u, set0 + w * G::BUFSTRIDE);
        __syncthreads();
#pragma unroll
        for (int s = 1; s < FftGeom<N, P>::S; s++) {
            load_slots<N, P>(x, u, set0 + w * G::BUFSTRIDE, s - 1);
            __syncthreads();
            stage_store<N, P, -1, false>(x, u, set0 + w * G::BUFSTRIDE, tw, s);
            __syncthreads();
        }
        or_p1_finish<N, P>(A, tw, jb, tid, f, x, set0);
    }
}

template <int N, int P>
__global__ __launch_bounds__((OrP1Geom<N, P>::NTHREADS)) void k_or_pass1(OrP1Args A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using G = OrP1Geom<N, P>;
    cf* lds = reinterpret_cast<cf*>(smem);
    constexpr int T = FftGeom<N, P>::T;
    // gridDim.y == 3: one field per block (a single texture is latency-bound: the three fields of a column job run as three
    // concurrent blocks, each recomputing the cheap h~); gridDim.y == 1: the block does the three fields one after the other
    // from ONE read of the spectrum and phase (a batched handle is bandwidth-bound: 24 instead of 41.5 B per texel read)
    const int tid = threadIdx.x, jb = blockIdx.x;
    const int f0 = gridDim.y == 1 ? 0 : (int)blockIdx.y, f1 = gridDim.y == 1 ? 3 : f0 + 1;
    {   // tile blockIdx.z of a batched handle
        const size_t toff = (size_t)blockIdx.z * N * N;
        A.initT += toff; A.phase_in += toff; A.phase_out += toff; A.E += 3 * toff;
    }
    const int w = tid / T, u = tid % T;
    TwStage<N, P, G::NTHREADS, false> tws;
    tws.load(A.TW, tid);
    const Twiddles tw = TwGeom<N, P>::view(A.TW, lds);
    cf* set0 = lds + G::TW_LDS;
    cf h[P], x[P];
    if (gridDim.y == 1) or_p1_animate<N, P, MW_OR_P1_CHUNK>(A, jb, tid, f0 == 0, h);  // one workgroup per column job: bandwidth-bound forms
    else or_p1_animate<N, P, 1>(A, jb, tid, f0 == 0, h);                                // one field per workgroup: the lone frame
    tws.store(lds, tid);  // behind the spectrum / phase requests; published by the first barrier
    for (int f = f0; f < f1; f++) {
        or_p1_build<N, P>(A, jb, tid, f, h, x);
        if (f != f0) __syncthreads();  // the previous field's final-pass reads of the buffers are done
        stage0_store<N, P, -1>(x, u, set0 + w * G::BUFSTRIDE);
        __syncthreads();
#pragma unroll
        for (int s = 1; s < FftGeom<N, P>::S; s++) {
            load_slots<N, P>(x, u, set0 + w * G::BUFSTRIDE, s - 1);
            __syncthreads();
            stage_store<N, P, -1, false>(x, u, set0 + w * G::BUFSTRIDE, tw, s);
            __syncthreads();
        }
        or_p1_finish<N, P>(A, tw, jb, tid, f, x, set0);
    }
}

// nframes consecutive frames of one ocean: grid (M/4 column jobs, 1, frame groups).  KEEP: the initial spectrum of the workgroup's
// points stays in registers over the frames of its group (else re-read per frame: an L2 hit after the first).
// (forcing 5 / 6 waves per SIMD with amdgpu_waves_per_eu: 44 / 108 B of scratch, 19.4 / 21.5 us per frame against 19.2: not kept)
template <int N, int P, bool KEEP, bool PACKED = false>
__global__ __launch_bounds__((OrP1Geom<N, P>::NTHREADS)) void k_or_pass1_steps(OrP1StepsArgs S) {
    constexpr int NF = PACKED ? 2 : 3;  // planes of the exchange buffer per frame
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using G = OrP1Geom<N, P>;
    cf* lds = reinterpret_cast<cf*>(smem);
    constexpr int T = FftGeom<N, P>::T;
    const int tid = threadIdx.x, jb = blockIdx.x;
    const int k0 = (int)blockIdx.z * S.group, k1 = (k0 + S.group < S.nframes) ? k0 + S.group : S.nframes;
    OrP1Args A = S.a;
    const int w = tid / T, u = tid % T;
    TwStage<N, P, G::NTHREADS, false> tws;
    tws.load(A.TW, tid);
    const Twiddles tw = TwGeom<N, P>::view(A.TW, lds);
    cf* set0 = lds + G::TW_LDS;
    float om[P], ph[P];
    f4 v[P], vn;
    const int fsel = PACKED ? (int)blockIdx.y : 0;  // packed plan: one field per workgroup (or_p1_steps_coeff)
    or_p1_steps_begin<N, P>(A, jb, tid, om, ph);
    float gain[PACKED ? P : 1];
    if constexpr (PACKED) {
        if (KEEP) or_p1_steps_coeff<N, P>(A, jb, tid, fsel, v, vn);
        or_p1_steps_gain<N, P>(A, jb, tid, fsel, gain);  // (the choppiness of this enqueue: A.c is fixed for its frames)
    }
    else { if (KEEP) or_p1_steps_spectrum<N, P>(A, jb, tid, v); }
    tws.store(lds, tid);  // behind the phase / spectrum requests; published by the first barrier
    for (int k = 0; k < k0; k++) or_p1_steps_advance<P>(om, ph, S.dt[k]);  // the chain over the frames of the groups before this one
    A.E += (size_t)NF * N * N * k0;
    for (int k = k0; k < k1; k++) {
        cf h[PACKED ? 1 : P], x[P];
        or_p1_steps_advance<P>(om, ph, S.dt[k]);
        if constexpr (PACKED) {
            if (!KEEP) or_p1_steps_coeff<N, P>(A, jb, tid, fsel, v, vn);
        } else {
            if (!KEEP) or_p1_steps_spectrum<N, P>(A, jb, tid, v);
            or_p1_steps_animate<P>(v, ph, h);
        }
        for (int f = PACKED ? fsel : 0; f < (PACKED ? fsel + 1 : 3); f++) {
            if constexpr (PACKED) or_p1_steps_build_split<N, P>(tid, f, gain, v, vn, ph, x);
            else or_p1_build<N, P>(A, jb, tid, f, h, x);
            if ((!PACKED && f != 0) || k != k0) __syncthreads();  // the previous field's final-pass reads of the buffers are done
            stage0_store<N, P, -1>(x, u, set0 + w * G::BUFSTRIDE);
            __syncthreads();
#pragma unroll
            for (int s = 1; s < FftGeom<N, P>::S; s++) {
                load_slots<N, P>(x, u, set0 + w * G::BUFSTRIDE, s - 1);
                __syncthreads();
                stage_store<N, P, -1, false>(x, u, set0 + w * G::BUFSTRIDE, tw, s);
                __syncthreads();
            }
            or_p1_finish<N, P>(A, tw, jb, tid, f, x, set0);
        }
        A.E += (size_t)NF * N * N;
    }
    if (k1 == S.nframes && fsel == 0) or_p1_steps_store_phase<N, P>(A, jb, tid, ph);  // the last group holds the phase after every frame
}

// the textures of frame `last` of a steps call become the handle's latest frame (mw_ocean_displace_mesh, the tile gather, ...): every array as
// float4 (M * M is a multiple of 4 and the frame offsets keep the 16-byte alignment), thread i copies element i of each array that has one
__global__ __launch_bounds__(256) void k_or_copy_frame(size_t MM, const float* h, const cf* d, const float* dg, const float* n, const float* w,
                                                       const float* hg, const float* da, float* oh, cf* od, float* odg, float* on, float* ow,
                                                       float* ohg, float* oda) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x, q = MM / 4;
    auto cp = [i](const void* src, void* dst) { reinterpret_cast<f4*>(dst)[i] = reinterpret_cast<const f4*>(src)[i]; };
    if (i < 3 * q) cp(n, on);
    if (i < 2 * q) cp(d, od);
    if (i < q) {
        cp(h, oh); cp(dg, odg); cp(w, ow);
        if (hg) { cp(hg, ohg); cp(da, oda); }
    }
}

// workgroup b of nb (a multiple of 8, else the identity) -> index in an order that gives XCD b % 8 one contiguous eighth of the indices
__device__ __forceinline__ unsigned or_xcd_band(unsigned b, unsigned nb) { return (nb % 8 == 0) ? (b % 8) * (nb / 8) + b / 8 : b; }
template <int N, int P>
__global__ __launch_bounds__((OrP2Geom<N, P>::NTHREADS)) void k_or_pass2(OrP2Args A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using G = OrP2Geom<N, P>;
    cf* lds = reinterpret_cast<cf*>(smem);
    constexpr int T = FftGeom<N, P>::T;
    // (row groups banded per XCD like the normal pass's rows, so that it would find these textures in its own L2: measured no gain, round 6)
    const int tid = threadIdx.x, ab = blockIdx.x;
    {   // tile blockIdx.z of a batched handle
        const size_t toff = (size_t)blockIdx.z * N * N;
        A.E += 3 * toff; A.height += toff; A.disp += toff; A.disp_g += toff;
        if (A.height_g) A.height_g += toff;
        if (A.disp_a) A.disp_a += toff;
    }
    TwStage<N, P, G::NTHREADS, false> tws;
    tws.load(A.TW, tid);
    const Twiddles tw = TwGeom<N, P>::view(A.TW, lds);
    cf* set0 = lds + G::TW_LDS;
    cf x[P];
    float dx[P];
    // grid.y = 0: hx then hz (their real parts leave interleaved as displacementTexture.rb); grid.y = 1: h
    const int k0 = blockIdx.y == 0 ? 0 : 2, k1 = blockIdx.y == 0 ? 2 : 3;
    for (int k = k0; k < k1; k++) {
        const int f = or_p2_field(k);
        if (k != k0) __syncthreads();
        or_p2_load<N, P>(A, ab, tid, f, x, set0);
        if (k == k0) tws.store(lds, tid);  // behind the first row requests; published by the barrier below
        __syncthreads();
#pragma unroll
        for (int s = 1; s < FftGeom<N, P>::S; s++) {
            // exact LDS layouts: a wave stays inside one row; padded layout: the load-side (row-interleaved) mapping
            const int um = XLay<N, P>::EXACT ? tid % FftGeom<N, P>::T : tid >> 2, rm = XLay<N, P>::EXACT ? tid / FftGeom<N, P>::T : tid & 3;
            load_slots<N, P>(x, um, set0 + rm * G::BUFSTRIDE, s - 1);
            __syncthreads();
            stage_store<N, P, -1, false>(x, um, set0 + rm * G::BUFSTRIDE, tw, s);
            __syncthreads();
        }
        or_p2_finish<N, P>(A, tw, ab, tid, f, x, dx, set0);
    }
}

// the packed plan's second pass: plane 0 = hx (-> displacement.r, .g), plane 1 = G (-> height.r + i displacement.b); one workgroup per 4 rows
template <int N, int P>
__global__ __launch_bounds__((OrP2Geom<N, P>::NTHREADS)) void k_or_pass2_packed(OrP2Args A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using G = OrP2Geom<N, P>;
    cf* lds = reinterpret_cast<cf*>(smem);
    const int tid = threadIdx.x, ab = blockIdx.x;
    {   // tile / frame blockIdx.z
        const size_t toff = (size_t)blockIdx.z * N * N;
        A.E += 2 * toff; A.height += toff; A.disp += toff; A.disp_g += toff;
    }
    TwStage<N, P, G::NTHREADS, false> tws;
    tws.load(A.TW, tid);
    const Twiddles tw = TwGeom<N, P>::view(A.TW, lds);
    cf* set0 = lds + G::TW_LDS;
    cf x[P];
    float dx[P];
    // gridDim.y == 2 (the lone frame: 256 row groups on 256 CUs, latency-bound): one field per workgroup, half the work on the critical path
    const bool split = gridDim.y == 2;
    const int k0 = split ? (int)blockIdx.y : 0, k1 = split ? k0 + 1 : 2;
    for (int k = k0; k < k1; k++) {
        if (k != k0) __syncthreads();
        or_p2_load<N, P>(A, ab, tid, k, x, set0);
        if (k == k0) tws.store(lds, tid);
        __syncthreads();
#pragma unroll
        for (int s = 1; s < FftGeom<N, P>::S; s++) {
            const int um = XLay<N, P>::EXACT ? tid % FftGeom<N, P>::T : tid >> 2, rm = XLay<N, P>::EXACT ? tid / FftGeom<N, P>::T : tid & 3;
            load_slots<N, P>(x, um, set0 + rm * G::BUFSTRIDE, s - 1);
            __syncthreads();
            stage_store<N, P, -1, false>(x, um, set0 + rm * G::BUFSTRIDE, tw, s);
            __syncthreads();
        }
        or_p2_finish<N, P>(A, tw, ab, tid, split ? 4 + k : (k == 0 ? 1 : 3), x, dx, set0);
    }
}

// F/OceanNormal.shader + F/WhiteCap.shader in one launch: WhiteCap reads _Bump at its own texel only (:38), so the thread
// that produced the normal goes straight on to the whitecap (its own global write is visible to itself).
template <bool NT>
__global__ __launch_bounds__(256) void k_or_normal_white(OrConsts c, const float* height, const cf* disp, const float* disp_g,
                                                         float* normal, float* white) {
    // XCD-aware: block b runs on XCD b % 8; give each XCD one contiguous band of texel rows, so that the +-1 and +-8 row
    // neighbours are hits in ITS L2 (round-robin rows made every XCD fetch its own copy: 29.5 B/texel for 16 needed)
    const unsigned blk = or_xcd_band(blockIdx.x, gridDim.x);
    int idx = blk * blockDim.x + threadIdx.x;
    {   // tile blockIdx.y of a batched handle
        const size_t toff = (size_t)blockIdx.y * c.M * c.M;
        height += toff; disp += toff; disp_g += toff; normal += 3 * toff; white += toff;
    }
    const int Q = c.M / 4;  // thread idx: texels 4 (idx % Q) .. + 3 of row idx / Q, from 16-byte loads
    if (idx >= c.M * Q) return;  // whole waves (M^2 / 4 is a multiple of 64)
    float n[4][3], w[4];
    or_normal_white_quad_compute(c, 4 * (idx % Q), idx / Q, height, disp, disp_g, n, w);
    f4 o;
    o.x = w[0]; o.y = w[1]; o.z = w[2]; o.w = w[3];
    mw_store_stream<NT>(reinterpret_cast<f4*>(white) + idx, o);  // 64 lanes x 16 B = 1 KiB contiguous
    // The normals: a lane owns 48 contiguous bytes (4 texels x 3), a wave 3 KiB (thread idx <-> texels 4 idx .. 4 idx + 3 of the row-major texture).
    // Stored straight from the lane every instruction writes 16-byte pieces 48 bytes apart -- a third of every line, left to the L2 to merge, and
    // slow with the non-temporal hint.  Turned through LDS inside the wave (as wave_store_3f4 does for the pond's vertices) every store
    // instruction writes 64 consecutive float4 = 1 KiB.
    __shared__ f4 tile[256 * 3];
    const int lane = threadIdx.x & 63;
    f4* wt = tile + (threadIdx.x - lane) * 3;
    f4 r0, r1, r2;
    r0.x = n[0][0]; r0.y = n[0][1]; r0.z = n[0][2]; r0.w = n[1][0];
    r1.x = n[1][1]; r1.y = n[1][2]; r1.z = n[2][0]; r1.w = n[2][1];
    r2.x = n[2][2]; r2.y = n[3][0]; r2.z = n[3][1]; r2.w = n[3][2];
    wt[lane * 3] = r0; wt[lane * 3 + 1] = r1; wt[lane * 3 + 2] = r2;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    f4* dst = reinterpret_cast<f4*>(normal) + (size_t)3 * (idx - lane);
#pragma unroll
    for (int j = 0; j < 3; j++) mw_store_stream<NT>(&dst[j * 64 + lane], wt[j * 64 + lane]);
}
static inline unsigned or_nw_blocks(size_t MM) { return (unsigned)((MM / 4 + 255) / 256); }

__global__ void k_or_pack_rgba(int M, const float* height, const float* height_g, const cf* disp, const float* disp_g,
                               const float* disp_a, const float* normal, const float* white, f4* H, f4* D, f4* Nn, f4* W) {
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)M * M) return;
    const size_t toff = (size_t)blockIdx.y * M * M;  // tile blockIdx.y
    or_pack_rgba_element(idx, height + toff, height_g + toff, disp + toff, disp_g + toff, disp_a + toff, normal + 3 * toff, white + toff,
                         H ? H + toff : nullptr, D ? D + toff : nullptr, Nn ? Nn + toff : nullptr, W ? W + toff : nullptr);
}
__global__ void k_or_displace_mesh(int M, int res, float unit_width, const float* height, const cf* disp, const float* normal,
                                   const float* white, float* vert, float* nrm, float* col) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= res * res) return;
    const size_t toff = (size_t)blockIdx.y * M * M, voff = (size_t)blockIdx.y * res * res;  // tile blockIdx.y
    or_mesh_vertex(M, res, unit_width, idx / res, idx % res, height + toff, disp + toff, normal + 3 * toff, white + toff, vert + 3 * voff,
                   nrm ? nrm + 3 * voff : nullptr, col ? col + voff : nullptr);
}

std::vector<cf> build_twiddle_table(int N, int P, int sgn);  // mistral_water.hip
int plan_points_host(int N);

// Every device buffer of an OrState, named once: the rows or_alloc allocates (in this order) and or_release frees.  `when` says which call
// brings a row: creation; the first call that wants Im h / Im Dz; a steps call -- always, for a texture kind the caller gave no
// destination for, or for the RGBA layout.
enum : unsigned {
    OR_B_HANDLE = 1u, OR_B_IMAG = 2u, OR_B_FR = 4u, OR_B_FR_HEIGHT = 8u, OR_B_FR_DISP = 16u, OR_B_FR_NORMAL = 32u, OR_B_FR_WHITE = 64u,
    OR_B_FR_IMAG = 128u, OR_B_FRAMES = 252u, OR_B_ALL = 255u
};
struct OrBuf { void** p; size_t bytes; unsigned when; };
constexpr int OR_NBUF = 22;
// tw_count: entries of the twiddle table; frames: capacity of the frame buffers (either may be 0 for a caller that only frees)
static inline void or_buffers(OrState& s, size_t tw_count, size_t frames, OrBuf (&b)[OR_NBUF]) {
    const size_t MM = (size_t)s.M * s.M, TM = MM * (size_t)s.tiles, FM = MM * frames;
    int n = 0;
    auto row = [&](auto*& p, size_t count, unsigned when) { b[n++] = OrBuf{(void**)&p, sizeof(*p) * count, when}; };
    row(s.initT, TM, OR_B_HANDLE); row(s.PQT, TM, OR_B_HANDLE); row(s.phaseT, TM, OR_B_HANDLE); row(s.phaseT2, TM, OR_B_HANDLE);
    row(s.omT, MM, OR_B_HANDLE); row(s.TW, tw_count, OR_B_HANDLE); row(s.E, 3 * TM, OR_B_HANDLE);
    row(s.out.height, TM, OR_B_HANDLE); row(s.out.disp, TM, OR_B_HANDLE); row(s.out.disp_g, TM, OR_B_HANDLE);
    row(s.out.normal, 3 * TM, OR_B_HANDLE); row(s.out.white, TM, OR_B_HANDLE);
    row(s.out.height_g, TM, OR_B_IMAG); row(s.out.disp_a, TM, OR_B_IMAG);
    row(s.fr_E, 3 * FM, OR_B_FR); row(s.fr.disp_g, FM, OR_B_FR);
    row(s.fr.height, FM, OR_B_FR_HEIGHT); row(s.fr.disp, FM, OR_B_FR_DISP); row(s.fr.normal, 3 * FM, OR_B_FR_NORMAL);
    row(s.fr.white, FM, OR_B_FR_WHITE); row(s.fr.height_g, FM, OR_B_FR_IMAG); row(s.fr.disp_a, FM, OR_B_FR_IMAG);
}
// the rows of `when` that are not there yet; false: a hipMalloc failed (what it did allocate stays, for or_free)
static inline bool or_alloc(OrState& s, unsigned when, size_t tw_count, size_t frames) {
    OrBuf b[OR_NBUF];
    or_buffers(s, tw_count, frames, b);
    for (const OrBuf& r : b)
        if ((r.when & when) && !*r.p && hipMalloc(r.p, r.bytes) != hipSuccess) return false;
    return true;
}
static inline void or_release(OrState& s, unsigned when) {  // (hipFree waits for the device)
    OrBuf b[OR_NBUF];
    or_buffers(s, 0, 0, b);
    for (const OrBuf& r : b)
        if (r.when & when) { hipFree(*r.p); *r.p = nullptr; }
}
static inline void or_free(OrState& s) {
    or_release(s, OR_B_ALL);
    s = OrState();
}

// RenderInitial() (S/OceanRenderer.cs:94-109): initialTexture from length / wind / amplitude, then the dispersion and spectrum tables on that
// length.  At creation the phase starts at 0 with it; after a parameter change (mw_ocean_reinit_spectrum) the phase textures and the normal
// pass's length stay.
static inline mw_status or_reinit(OrState& s, float length, float wind_x, float wind_y, float amplitude, uint64_t seed, hipStream_t st,
                                  bool restart_phase = false) {
    const size_t MM = (size_t)s.M * s.M;
    s.c.length = length;
    k_or_init<<<dim3((unsigned)((MM + 255) / 256), s.tiles), dim3(256), 0, st>>>(s.M, length, wind_x, wind_y, amplitude / 10000.f,
                                                                                s.c.gravity, seed, s.initT, restart_phase ? s.phaseT : nullptr);
    k_or_omega<<<dim3((unsigned)((MM + 255) / 256)), dim3(256), 0, st>>>(s.c, s.omT);
    k_or_prep<<<dim3((unsigned)((MM + 255) / 256), s.tiles), dim3(256), 0, st>>>(s.M, s.initT, s.PQT);
    if (hipGetLastError() != hipSuccess) return fail(MW_EDEVICE, "k_or_init launch failed");
    return MW_OK;
}
static inline mw_status or_create(OrState& s, const mw_params& p, int M, hipStream_t st, int tiles = 1) {
    s.M = M;
    s.tiles = tiles;
    s.c.M = M; s.c.length = p.length; s.c.gravity = p.gravity; s.c.choppiness = p.choppiness; s.c.normal_length = p.length;
    s.mult = p.mult;
    std::vector<cf> tab = build_twiddle_table(M, plan_points_host(M), -1);
    if (!or_alloc(s, OR_B_HANDLE, tab.size(), 0)) return fail(MW_ENOMEM, "OceanRenderer: hipMalloc failed");
    if (hipMemcpy(s.TW, tab.data(), sizeof(cf) * tab.size(), hipMemcpyHostToDevice) != hipSuccess) return fail(MW_EDEVICE, "twiddle upload failed");
    return or_reinit(s, p.length, p.wind_x, p.wind_y, p.amplitude, p.seed, st, true);
}
// Im h and Im Dz of the latest frame: allocated by the first call that delivers the RGBA layout
static inline mw_status or_imag_planes(OrState& s) {
    if (s.out.height_g) return MW_OK;
    return or_alloc(s, OR_B_IMAG, 0, 0) ? MW_OK : fail(MW_ENOMEM, "OceanRenderer: hipMalloc failed");
}
// the planar-texture plan of a call: two transforms per frame where the identity holds (or_prep_element), else the shaders' three
// (4096^2 textures keep three: their 1024-thread P = 16 workgroups have 128 registers per lane, and two animated spectra at once spill --
// one GenerateTexture() 545 -> 637 us; 2048^2: 127 -> 110 us, 4 / 8 tiles per call 24.0 / 25.1 -> 24.3 / 23.3 us per tile-frame)
// imag: the call delivers Im h and Im Dz (the RGBA layout): they are channels of the targets, so it runs the three-transform plan
static inline bool or_use_packed(const OrState& s, bool imag) {
    return MW_OR_PACKED != 0 && sw(SW_OR_PACKED) != 0 && !imag && s.phase_sym && s.M < MW_OR_PACKED_MAX_M;
}

// phase texture <-> host order (texel (px,py) at py*M + px); the device keeps it transposed
__global__ void k_or_phase_transpose(int M, const float* src, float* dst) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * M) return;
    const size_t toff = (size_t)blockIdx.y * M * M;  // tile blockIdx.y
    (dst + toff)[idx] = (src + toff)[(size_t)(idx % M) * M + idx / M];
}

#ifndef MW_OR_STREAM_E_TILES
#define MW_OR_STREAM_E_TILES 2
#endif
#ifndef MW_OR_BIG_N
#define MW_OR_BIG_N 2048  // from this texture size up ONE tile is what several 1024^2 tiles are: it fills the device and its exchange buffer the caches
#endif
// a call is "bandwidth-bound" (three fields per pass-1 block from one read of the spectrum, streaming stores) when it carries several tiles or
// one big one; a single 1024^2 texture is latency-bound (one field per block, cacheable stores)
#ifndef MW_OR_STREAM_BIG_N
#define MW_OR_STREAM_BIG_N MW_OR_BIG_N
#endif
static inline bool or_call_is_big(const OrState& s) { return s.tiles >= MW_OR_STREAM_E_TILES || s.M >= MW_OR_STREAM_BIG_N; }
// all fields of a column job in one pass-1 workgroup (else one field per workgroup: the lone frame)
static inline bool or_all_fields(const OrState& s) { return s.tiles > 1 || s.M >= MW_OR_BIG_N; }
// The arguments of a spectrum launch at the handle's current phase: (initT, PQT) the spectrum it animates (the handle's, or the velocity's
// weighted one), phase_out where the advanced phase goes, E the exchange buffer it fills.
static inline OrP1Args or_p1_args(const OrState& s, const f4* initT, const f4* PQT, float* phase_out, cf* E, float dt, bool stream_E) {
    OrP1Args A;
    A.initT = initT; A.PQT = PQT; A.omT = s.omT; A.phase_in = s.phaseT; A.phase_out = phase_out; A.TW = s.TW; A.E = E; A.c = s.c; A.dt = dt;
    A.stream_E = stream_E ? 1 : 0;
    return A;
}
// ... and of the second pass from E into the set t (a planar set: no Im h / Im Dz written)
static inline OrP2Args or_p2_args(const OrState& s, const cf* E, const OrTex& t) {
    OrP2Args A;
    A.E = E; A.TW = s.TW; A.height = t.height; A.disp = t.disp; A.disp_g = t.disp_g; A.c = s.c;
    A.height_g = t.height_g; A.disp_a = t.disp_a;
    return A;
}
template <int N>
static hipError_t or_launch_passes(OrState& s, float dt, bool imag, hipStream_t st, hipEvent_t* ev = nullptr) {
    constexpr int P = Plan<N>::P;
    static AttrOnce attr1, attr2;
    hipError_t e = attr1.set(reinterpret_cast<const void*>(&k_or_pass1<N, P>), OrP1Geom<N, P>::LDS_BYTES);
    if (e == hipSuccess) e = attr2.set(reinterpret_cast<const void*>(&k_or_pass2<N, P>), OrP2Geom<N, P>::LDS_BYTES);
    if (e != hipSuccess) return e;
    const OrP1Args A1 = or_p1_args(s, s.initT, s.PQT, s.phaseT2, s.E, dt, or_call_is_big(s));
    const OrP2Args A2 = or_p2_args(s, s.E, imag ? s.out : s.out.real_only());
    constexpr int NT1 = OrP1Geom<N, P>::NTHREADS, LB1 = OrP1Geom<N, P>::LDS_BYTES;
    constexpr int NT2 = OrP2Geom<N, P>::NTHREADS, LB2 = OrP2Geom<N, P>::LDS_BYTES;
    const bool packed = or_use_packed(s, imag), all_fields = or_all_fields(s);
    if constexpr (N < MW_OR_PACKED_MAX_M) if (packed) {
        static AttrOnce attr1p, attr2p;
        e = attr1p.set(reinterpret_cast<const void*>(&k_or_pass1_packed<N, P>), LB1);
        if (e == hipSuccess) e = attr2p.set(reinterpret_cast<const void*>(&k_or_pass2_packed<N, P>), LB2);
        if (e != hipSuccess) return e;
        if (ev) hipEventRecord(ev[0], st);
        k_or_pass1_packed<N, P><<<dim3(N / 4, all_fields ? 1 : 2, s.tiles), dim3(NT1), LB1, st>>>(A1);
        if (ev) hipEventRecord(ev[1], st);
        std::swap(s.phaseT, s.phaseT2);
        k_or_pass2_packed<N, P><<<dim3(N / 4, all_fields ? 1 : 2, s.tiles), dim3(NT2), LB2, st>>>(A2);  // lone frame: one field per workgroup
        if (ev) hipEventRecord(ev[2], st);
        return hipGetLastError();
    }
    if (ev) hipEventRecord(ev[0], st);
    k_or_pass1<N, P><<<dim3(N / 4, all_fields ? 1 : 3, s.tiles), dim3(NT1), LB1, st>>>(A1);
    if (ev) hipEventRecord(ev[1], st);
    std::swap(s.phaseT, s.phaseT2);
    k_or_pass2<N, P><<<dim3(N / 4, 2, s.tiles), dim3(NT2), LB2, st>>>(A2);
    if (ev) hipEventRecord(ev[2], st);
    return hipGetLastError();
}

// one GenerateTexture(): results land in s.out (imag: Im h and Im Dz too); optional device destinations receive copies
// ev (measurement hook, 5 events): recorded before pass 1 and after pass 1, pass 2, the normal / whitecap pass and the copies
static inline mw_status or_generate(OrState& s, float delta_time, bool imag, float* d_height, float* d_disp, float* d_normal, float* d_white,
                                    hipStream_t st, hipEvent_t* ev = nullptr) {
    const float dt = delta_time * s.mult;  // S/OceanRenderer.cs:223
    const mw_status r = imag ? or_imag_planes(s) : MW_OK;
    if (r != MW_OK) return r;
    hipError_t e = hipSuccess;
    MW_FOR_SIZE(s.M, return fail(MW_EINVAL, "OceanRenderer: unsupported texture size"), e = or_launch_passes<NN>(s, dt, imag, st, ev));
    if (e != hipSuccess) return fail(MW_EDEVICE, std::string("OceanRenderer pass launch: ") + hipGetErrorString(e));
    const size_t MM = (size_t)s.M * s.M, TM = MM * (size_t)s.tiles;
    const unsigned nb = or_nw_blocks(MM);
    const OrTex& o = s.out;
    if (or_call_is_big(s)) k_or_normal_white<true><<<dim3(nb, s.tiles), dim3(256), 0, st>>>(s.c, o.height, o.disp, o.disp_g, o.normal, o.white);
    else k_or_normal_white<false><<<dim3(nb, s.tiles), dim3(256), 0, st>>>(s.c, o.height, o.disp, o.disp_g, o.normal, o.white);
    if (hipGetLastError() != hipSuccess) return fail(MW_EDEVICE, "OceanRenderer normal/white launch failed");
    if (ev) hipEventRecord(ev[3], st);
    s.have_frame = true;
    hipError_t ce = hipSuccess;
    if (d_height && ce == hipSuccess) ce = hipMemcpyAsync(d_height, o.height, TM * 4, hipMemcpyDeviceToDevice, st);
    if (d_disp && ce == hipSuccess) ce = hipMemcpyAsync(d_disp, o.disp, TM * 8, hipMemcpyDeviceToDevice, st);
    if (d_normal && ce == hipSuccess) ce = hipMemcpyAsync(d_normal, o.normal, TM * 12, hipMemcpyDeviceToDevice, st);
    if (d_white && ce == hipSuccess) ce = hipMemcpyAsync(d_white, o.white, TM * 4, hipMemcpyDeviceToDevice, st);
    if (ce != hipSuccess) return fail(MW_EDEVICE, std::string("OceanRenderer result copy: ") + hipGetErrorString(ce));
    if (ev) hipEventRecord(ev[4], st);
    return MW_OK;
}

// ---- nframes consecutive GenerateTexture() calls in one enqueue ------------------------------------------------------------------
// frame buffers of the handle: the exchange buffer and disp.g for `n` frames, plus every texture the caller gave no destination for
static inline mw_status or_frames_reserve(OrState& s, int n, const bool (&need)[4], bool imag) {
    if (n > s.frames_cap) {  // grow: drop everything, the arrays come back below at the new size
        or_release(s, OR_B_FRAMES);
        s.frames_cap = 0; s.frames_last = 0;
    }
    const size_t cap = (size_t)(s.frames_cap ? s.frames_cap : n);
    const unsigned when = OR_B_FR | (need[0] ? OR_B_FR_HEIGHT : 0u) | (need[1] ? OR_B_FR_DISP : 0u) | (need[2] ? OR_B_FR_NORMAL : 0u) |
                          (need[3] ? OR_B_FR_WHITE : 0u) | (imag ? OR_B_FR_IMAG : 0u);
    if (!or_alloc(s, when, 0, cap)) {
        (void)hipGetLastError();
        return fail(MW_ENOMEM, "OceanRenderer: hipMalloc of the frame buffers failed");
    }
    s.frames_cap = (int)cap;
    return MW_OK;
}
#ifndef MW_OR_FRAME_GROUPS
#define MW_OR_FRAME_GROUPS 4  // frame groups of a steps call = workgroups per column job (see k_or_pass1_steps)
#endif
#ifndef MW_OR_FRAME_GROUPS_PACKED
#define MW_OR_FRAME_GROUPS_PACKED 2  // the packed plan has two workgroups per column job and group already (one per field): 1 / 2 / 3 / 4 groups measured
#endif                               // 18.9 / 18.6 / 19.8 / 19.3 us per frame at 32 frames per enqueue
#ifndef MW_OR_STEPS_CHUNK
#define MW_OR_STEPS_CHUNK 8  // frames per pass-2 / normal-pass launch pair at 1024^2 (scaled with the texture area)
#endif
static inline int or_steps_chunk(int M) {
    const long long c = (long long)MW_OR_STEPS_CHUNK * 1024 * 1024 / ((long long)M * M);
    return c < 1 ? 1 : (c > MW_OR_MAX_FRAMES ? MW_OR_MAX_FRAMES : (int)c);
}
static inline int or_steps_chunks(int M, int n) { const int c = or_steps_chunk(M); return (n + c - 1) / c; }
#ifndef MW_OR_STEPS_MAX_N
#define MW_OR_STEPS_MAX_N 2048  // above: the 1024-thread P = 16 workgroup has 128 VGPRs per lane, no room for a chain in registers
#endif
// f: where the n frames go (the frame buffers, or the caller's arrays for the kinds it gave)
template <int N, bool PACKED>
static hipError_t or_launch_steps(OrState& s, const float* dt, int n, const OrTex& f, hipStream_t st, hipEvent_t* ev = nullptr) {
    constexpr int P = Plan<N>::P, NF = PACKED ? 2 : 3;
    // KEEP: (h0, h0c) -- and in the packed plan (P, Q) -- of a workgroup's points stay in registers over its frames (P = 16: no registers to spare)
    constexpr bool KEEP = P <= 8;
    static AttrOnce attr1, attr2;
    {
        hipError_t e;
        if constexpr (PACKED) e = attr2.set(reinterpret_cast<const void*>(&k_or_pass2_packed<N, P>), OrP2Geom<N, P>::LDS_BYTES);
        else e = attr2.set(reinterpret_cast<const void*>(&k_or_pass2<N, P>), OrP2Geom<N, P>::LDS_BYTES);
        if (e != hipSuccess) return e;
    }
    constexpr int NT1 = OrP1Geom<N, P>::NTHREADS, LB1 = OrP1Geom<N, P>::LDS_BYTES;
    if (ev) hipEventRecord(ev[0], st);
    constexpr int NT2 = OrP2Geom<N, P>::NTHREADS, LB2 = OrP2Geom<N, P>::LDS_BYTES;
    const size_t MM = (size_t)N * N;
    const int chunk = or_steps_chunk(N);
    // pass 2 and the normal / whitecap pass of the frames [c0, c0 + cn)
    auto rest = [&](int c0, int cn, int j) {
        const OrTex c = f.at(MM * (size_t)c0);
        const OrP2Args B2 = or_p2_args(s, s.fr_E + NF * MM * (size_t)c0, c);
        if constexpr (PACKED) k_or_pass2_packed<N, P><<<dim3(N / 4, 1, cn), dim3(NT2), LB2, st>>>(B2);
        else k_or_pass2<N, P><<<dim3(N / 4, 2, cn), dim3(NT2), LB2, st>>>(B2);
        if (ev) hipEventRecord(ev[2 + 3 * j], st);
        k_or_normal_white<true><<<dim3(or_nw_blocks(MM), cn), dim3(256), 0, st>>>(s.c, c.height, c.disp, c.disp_g, c.normal, c.white);
        if (ev) hipEventRecord(ev[3 + 3 * j], st);
    };
    // Pass 2 and the normal / whitecap pass alternate over chunks of frames: the height / displacement textures a chunk writes (16 B per texel
    // and frame) are still in the 256-MB Infinity Cache when the normal pass reads them back.  Behind 32 frames of pass-2 output (512 MB at
    // 1024^2) every read of the normal pass went to HBM: 9.1 us per frame against 7.2 from the cache (chunks of 4 / 8 / 16 / 32 frames:
    // 21.9 / 21.8 / 23.2 / 23.3 us per frame).
    if constexpr (N <= MW_OR_STEPS_MAX_N) {
        hipError_t e = attr1.set(reinterpret_cast<const void*>(&k_or_pass1_steps<N, P, KEEP, PACKED>), LB1);
        if (e != hipSuccess) return e;
        OrP1StepsArgs S;
        S.a = or_p1_args(s, s.initT, s.PQT, s.phaseT2, s.fr_E, 0.f, true);
        for (int k = 0; k < MW_OR_MAX_FRAMES; k++) S.dt[k] = k < n ? dt[k] : 0.f;
        S.nframes = n;
        // ONE spectrum launch over all frames: per chunk (so that pass 2 would find the exchange buffer in the cache) it ran 195 -> 283 us per 32
        // frames and pass 2 no faster -- the exchange buffer is written with streaming stores and does not stay
        int groups = PACKED ? MW_OR_FRAME_GROUPS_PACKED : MW_OR_FRAME_GROUPS;
        if (groups > n) groups = n;
        S.group = (n + groups - 1) / groups;
        groups = (n + S.group - 1) / S.group;
        k_or_pass1_steps<N, P, KEEP, PACKED><<<dim3(N / 4, PACKED ? 2 : 1, groups), dim3(NT1), LB1, st>>>(S);
        for (int c0 = 0, j = 0; c0 < n; c0 += chunk, j++) {
            if (ev) hipEventRecord(ev[1 + 3 * j], st);
            rest(c0, (n - c0 < chunk) ? n - c0 : chunk, j);
        }
        std::swap(s.phaseT, s.phaseT2);
    } else {  // one bandwidth-bound spectrum launch per frame (each already fills the device)
        hipError_t e;
        if constexpr (PACKED) e = attr1.set(reinterpret_cast<const void*>(&k_or_pass1_packed<N, P>), LB1);
        else e = attr1.set(reinterpret_cast<const void*>(&k_or_pass1<N, P>), LB1);
        if (e != hipSuccess) return e;
        for (int c0 = 0, j = 0; c0 < n; c0 += chunk, j++) {
            const int cn = (n - c0 < chunk) ? n - c0 : chunk;
            for (int k = c0; k < c0 + cn; k++) {
                const OrP1Args A1 = or_p1_args(s, s.initT, s.PQT, s.phaseT2, s.fr_E + (size_t)NF * N * N * k, dt[k], true);
                if constexpr (PACKED) k_or_pass1_packed<N, P><<<dim3(N / 4, 1, 1), dim3(NT1), LB1, st>>>(A1);
                else k_or_pass1<N, P><<<dim3(N / 4, 1, 1), dim3(NT1), LB1, st>>>(A1);
                std::swap(s.phaseT, s.phaseT2);
            }
            if (ev) hipEventRecord(ev[1 + 3 * j], st);
            rest(c0, cn, j);
        }
    }
    return hipGetLastError();
}
// frames k = 0 .. n-1 advance the phase by delta_time[k] * mult one after the other, exactly as n calls of or_generate would; device
// destinations are [n][M*M*...] (NULL: the frame stays in the handle's own frame buffers).  The handle's latest-frame textures
// (s.out) receive frame n-1.
static inline mw_status or_generate_steps(OrState& s, const float* delta_time, int n, bool imag, float* d_height, float* d_disp, float* d_normal,
                                          float* d_white, hipStream_t st, hipEvent_t* ev = nullptr) {
    if (s.tiles != 1) return fail(MW_ESTATE, "generate_texture_steps: a batched handle (mw_ocean_create_batch) advances one frame per call");
    if (n < 1 || n > MW_OR_MAX_FRAMES) return fail(MW_EINVAL, "generate_texture_steps: nframes out of range");
    const size_t MM = (size_t)s.M * s.M;
    mw_status r = imag ? or_imag_planes(s) : MW_OK;
    if (r != MW_OK) return r;
    const bool need[4] = {!d_height, !d_disp, !d_normal, !d_white};
    if ((r = or_frames_reserve(s, n, need, imag)) != MW_OK) return r;
    float dt[MW_OR_MAX_FRAMES];
    for (int k = 0; k < n; k++) dt[k] = delta_time[k] * s.mult;  // S/OceanRenderer.cs:223
    OrTex f = imag ? s.fr : s.fr.real_only();
    if (d_height) f.height = d_height;
    if (d_disp) f.disp = reinterpret_cast<cf*>(d_disp);
    if (d_normal) f.normal = d_normal;
    if (d_white) f.white = d_white;
    hipError_t e = hipSuccess;
    const bool packed = or_use_packed(s, imag);  // (false from MW_OR_PACKED_MAX_M up: no packed instantiation there)
    MW_FOR_SIZE(s.M, return fail(MW_EINVAL, "OceanRenderer: unsupported texture size"),
                e = packed ? or_launch_steps<NN, (NN < MW_OR_PACKED_MAX_M)>(s, dt, n, f, st, ev) : or_launch_steps<NN, false>(s, dt, n, f, st, ev));
    if (e != hipSuccess) return fail(MW_EDEVICE, std::string("OceanRenderer steps launch: ") + hipGetErrorString(e));
    const OrTex l = f.at((size_t)(n - 1) * MM), &o = s.out;
    k_or_copy_frame<<<dim3((unsigned)((3 * MM / 4 + 255) / 256)), dim3(256), 0, st>>>(MM, l.height, l.disp, l.disp_g, l.normal, l.white, l.height_g, l.disp_a,
                                                                                     o.height, o.disp, o.disp_g, o.normal, o.white, o.height_g, o.disp_a);
    if (hipGetLastError() != hipSuccess) return fail(MW_EDEVICE, "OceanRenderer normal/white launch failed");
    if (ev) hipEventRecord(ev[1 + 3 * or_steps_chunks(s.M, n)], st);
    s.have_frame = true;
    return MW_OK;
}

// n consecutive frames at the handle's choppiness: the lone-frame plan at n == 1 (latency-bound launch forms; its textures are the handle's own
// s.out), else the steps plan (s.fr).  Planar (d: height, displacement, normal, whitecap as floats; a NULL kind stays in the handle) or, rgba,
// delivered as the reference's four ARGBFloat render targets ([n][M*M*4] each, any may be NULL).  ev: the measurement hook's events.
static inline mw_status or_frames(OrState& s, float choppiness, const float* delta_time, int n, bool rgba, void* const (&d)[4], hipStream_t st,
                                  hipEvent_t* ev = nullptr) {
    s.c.choppiness = choppiness;
    float* const p[4] = {rgba ? nullptr : (float*)d[0], rgba ? nullptr : (float*)d[1], rgba ? nullptr : (float*)d[2], rgba ? nullptr : (float*)d[3]};
    const mw_status r = n == 1 ? or_generate(s, delta_time[0], rgba, p[0], p[1], p[2], p[3], st, ev)
                               : or_generate_steps(s, delta_time, n, rgba, p[0], p[1], p[2], p[3], st, ev);
    if (r != MW_OK || !rgba) return r;
    const size_t MM = (size_t)s.M * s.M;
    const OrTex& t = n == 1 ? s.out : s.fr;
    k_or_pack_rgba<<<dim3((unsigned)((MM + 255) / 256), n == 1 ? s.tiles : n), dim3(256), 0, st>>>(s.M, t.height, t.height_g, t.disp, t.disp_g, t.disp_a, t.normal,
                                                                                              t.white, (f4*)d[0], (f4*)d[1], (f4*)d[2], (f4*)d[3]);
    if (hipGetLastError() != hipSuccess) return fail(MW_EDEVICE, "k_or_pack_rgba launch failed");
    return MW_OK;
}

// The Dispersion pass alone (F/Dispersion.shader:32-41) for n frames: the phase texture after n GenerateTexture() calls with these delta times,
// no textures produced -- the same or_phase_step chain per texel, so a handle advanced this way continues bit for bit like one that rendered the
// frames.  How a rank of a multi-GPU job seeks to ITS block of a frame sequence (time-steps shard across devices; in this
// semantics only the phase links them), and how a recorder skips frames.
struct OrAdvanceArgs {
    float dt[MW_OR_MAX_FRAMES];
    int n;
};
__global__ __launch_bounds__(256) void k_or_advance(size_t MM, const float* omT, float* phase, OrAdvanceArgs A) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= MM) return;
    const float om = omT[i];
    float ph = phase[i + (size_t)blockIdx.y * MM];  // tile blockIdx.y
    for (int k = 0; k < A.n; k++) ph = or_phase_step(om, ph, A.dt[k]);
    phase[i + (size_t)blockIdx.y * MM] = ph;
}
static inline mw_status or_advance_phase(OrState& s, const float* delta_time, int n, hipStream_t st) {
    const size_t MM = (size_t)s.M * s.M;
    for (int k0 = 0; k0 < n; k0 += MW_OR_MAX_FRAMES) {
        OrAdvanceArgs A;
        A.n = (n - k0 < MW_OR_MAX_FRAMES) ? n - k0 : MW_OR_MAX_FRAMES;
        for (int k = 0; k < MW_OR_MAX_FRAMES; k++) A.dt[k] = k < A.n ? delta_time[k0 + k] * s.mult : 0.f;  // S/OceanRenderer.cs:223
        k_or_advance<<<dim3((unsigned)((MM + 255) / 256), s.tiles), dim3(256), 0, st>>>(MM, s.omT, s.phaseT, A);
    }
    if (hipGetLastError() != hipSuccess) return fail(MW_EDEVICE, "k_or_advance launch failed");
    return MW_OK;
}

// the ocean material's vertex stage on the res x res mesh, from the textures of the latest GenerateTexture()
static inline mw_status or_displace_mesh(OrState& s, int res, float unit_width, float* d_vert, float* d_nrm, float* d_col,
                                         hipStream_t st) {
    if (!s.have_frame) return fail(MW_ESTATE, "displace_mesh: no GenerateTexture() yet");
    const int nv = res * res;
    k_or_displace_mesh<<<dim3((unsigned)((nv + 255) / 256), s.tiles), dim3(256), 0, st>>>(s.M, res, unit_width, s.out.height,
                                                                                 s.out.disp, s.out.normal, s.out.white,
                                                                                 d_vert, d_nrm, d_col);
    if (hipGetLastError() != hipSuccess) return fail(MW_EDEVICE, "k_or_displace_mesh launch failed");
    return MW_OK;
}

}  // namespace mw
