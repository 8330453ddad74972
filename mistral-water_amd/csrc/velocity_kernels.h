// velocity_kernels.h -- surface velocity (mw_ocean_velocity, include/mistral_water.h): the time derivative of the displaced mesh.
//
// Every output of a frame is linear in the initial spectrum, and time enters only through the phase factors:
//   FFTMesh (S/FFTMesh.cs:178-190)       h~(k, t) = h0(k) e^{i w t} + h0c(k) e^{-i w t}           (htilde: h0conj times c1 = e^{-i w t})
//   OceanRenderer (F/Spectrum.shader:45) h~(k)    = init.rg e^{i phi} + init.ba e^{-i phi},  d phi / dt = w(texel)
// so d h~ / dt = (i w h0) e^{i w t} + (-i w h0c) e^{-i w t}: the frame pipeline run on the weighted spectrum (i w h0, -i w h0c) -- the
// second half takes -i w because it is multiplied by e^{-i w t} as it is, not conjugated -- is its own time derivative, through every
// transform path (Stockham FFT, chirp-z, GEMM) and the packed plans.  The FFT path's prep pairs index (i, j) with its mirror under
// ONE w, the OceanRenderer's packed plan pairs texels under one phase: both hold because w (and the phase) is mirror-symmetric bit for
// bit (tests/test_velocity_cpu.py::test_omega_is_mirror_symmetric).
//
// What reaches the caller is the derivative of the vertex, without the rest coordinate:
//   FFTMesh        vertex = (x - chop Dx, h, z - chop Dz)  ->  velocity = (-chop dDx/dt, dh/dt, -chop dDz/dt)   per unit of t
//   OceanRenderer  vertex = rest + (Dx, h, Dz) / 8 sampled  ->  velocity = (dDx/dt, dh/dt, dDz/dt) / 8 sampled  per second of delta_time
// The frame kernels write rest_coord(N, unit_width, a) - chop Dx; run with unit_width = 0 the rest coordinate is +-0 and the difference
// IS -chop Dx, rounded once -- no position is subtracted afterwards, which would cancel the digits the velocity is made of.
#pragma once
#include "mw_math.h"
// MW_VEL_NO_KERNELS: a second translation unit (water_column.hip) wants velocity_weight alone; the kernels and VelState are mistral_water.hip's
#if defined(__HIPCC__) && !defined(MW_VEL_NO_KERNELS)
#include "direct_kernels.h"
#include "ocean_renderer_device.h"
#endif

namespace mw {

// (h0, h0c) -> (i w h0, -i w h0c)
MW_HD void velocity_weight(float w, cf a, cf b, cf* va, cf* vb) {
    *va = mk(-(w * a.y), w * a.x);
    *vb = mk(w * b.y, -(w * b.x));
}

#if defined(__HIPCC__) && !defined(MW_VEL_NO_KERNELS)
// FFTMesh: the weighted spectrum, w = omega_f32 of the same index -- the value the frame kernels' Om table and omega_t_f32 hold
__global__ void k_velocity_spectrum(int N, float length, float gravity, const cf* h0, const cf* h0c, cf* vh0, cf* vh0c) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * N) return;
    velocity_weight(omega_f32(N, length, gravity, idx / N, idx % N), h0[idx], h0c[idx], &vh0[idx], &vh0c[idx]);
}
// OceanRenderer: initT = (init.rg, init.ba) [px][py], weighted with d phi / d delta_time = omega * mult (the phase advances by
// omega * delta_time * mult, S/OceanRenderer.cs:223), omega from the or_omega table of the same (transposed) layout
__global__ void k_or_velocity_init(int M, const float* omT, float mult, const f4* initT, f4* vinitT) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * M) return;
    const f4 v = initT[idx];
    cf a, b;
    velocity_weight(smul(omT[idx], mult), mk(v.x, v.y), mk(v.z, v.w), &a, &b);
    f4 o;
    o.x = a.x; o.y = a.y; o.z = b.x; o.w = b.y;
    vinitT[idx] = o;
}
// FFTMesh direct-sum paths (chirp-z, GEMM): their assembly kernels leave (dDx/dt, dDz/dt) in hds and dh/dt in vertex.y; the horizontal
// components are formed as the FFT path forms them with a zero rest coordinate (0 - chop D), in place
__global__ void k_velocity_from_hds(int N, float choppiness, const cf* hds, float* vel) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * N) return;
    const cf d = hds[idx];
    vel[3 * idx + 0] = ssub(0.f, smul(d.x, choppiness));
    vel[3 * idx + 2] = ssub(0.f, smul(d.y, choppiness));
}

// the velocity buffers of a handle, allocated on first use and freed with it (vel_free); `ready` says the weighted spectrum
// (and what is derived from it) belongs to the handle's current spectrum -- cleared by every entry point that replaces the spectrum
struct VelState {
    bool ready = false;
    // FFTMesh: the weighted spectrum, its k_prep tables (FFT path), and the normals / whitecap the frame kernels also write
    FmSpectrum sp;
    float *norm = nullptr, *white = nullptr;
    // OceanRenderer: weighted initial spectrum and its (P, Q), the phase the spectrum kernel stores (unchanged: dt = 0), the exchange
    // buffer and the rate textures of pass 2
    f4 *initT = nullptr, *PQT = nullptr;
    float* phase = nullptr;
    cf* E = nullptr;
    float *height = nullptr, *disp_g = nullptr;
    cf* disp = nullptr;
    // per-vertex velocity of the query entry points, [R*R][3]
    float* vert = nullptr;
};
static inline void vel_free(VelState& v) {
    fm_spectrum_free(v.sp); hipFree(v.norm); hipFree(v.white);
    hipFree(v.initT); hipFree(v.PQT); hipFree(v.phase); hipFree(v.E); hipFree(v.height); hipFree(v.disp_g); hipFree(v.disp); hipFree(v.vert);
    v = VelState();
}

// OceanRenderer: the passes of or_launch_passes on the weighted initial spectrum, at the handle's CURRENT phase (dt = 0: or_phase_step
// returns the phase it is given), into the velocity buffers; the same plan (packed or three transforms) and launch forms as a frame.
// Nothing of the handle is written: the phase goes to v.phase, the textures to v.height / v.disp.
template <int N>
static hipError_t or_velocity_passes(const OrState& s, VelState& v, hipStream_t st) {
    constexpr int P = Plan<N>::P;
    constexpr int NT1 = OrP1Geom<N, P>::NTHREADS, LB1 = OrP1Geom<N, P>::LDS_BYTES;
    constexpr int NT2 = OrP2Geom<N, P>::NTHREADS, LB2 = OrP2Geom<N, P>::LDS_BYTES;
    const OrP1Args A1 = or_p1_args(s, v.initT, v.PQT, v.phase, v.E, 0.f, or_call_is_big(s));
    OrTex rate;
    rate.height = v.height; rate.disp = v.disp; rate.disp_g = v.disp_g;
    const OrP2Args A2 = or_p2_args(s, v.E, rate);
    const bool all_fields = or_all_fields(s);
    static AttrOnce attr1, attr2;
    if constexpr (N < MW_OR_PACKED_MAX_M) if (or_use_packed(s, false)) {
        hipError_t e = attr1.set(reinterpret_cast<const void*>(&k_or_pass1_packed<N, P>), LB1);
        if (e == hipSuccess) e = attr2.set(reinterpret_cast<const void*>(&k_or_pass2_packed<N, P>), LB2);
        if (e != hipSuccess) return e;
        k_or_pass1_packed<N, P><<<dim3(N / 4, all_fields ? 1 : 2, 1), dim3(NT1), LB1, st>>>(A1);
        k_or_pass2_packed<N, P><<<dim3(N / 4, all_fields ? 1 : 2, 1), dim3(NT2), LB2, st>>>(A2);
        return hipGetLastError();
    }
    static AttrOnce attr1t, attr2t;
    hipError_t e = attr1t.set(reinterpret_cast<const void*>(&k_or_pass1<N, P>), LB1);
    if (e == hipSuccess) e = attr2t.set(reinterpret_cast<const void*>(&k_or_pass2<N, P>), LB2);
    if (e != hipSuccess) return e;
    k_or_pass1<N, P><<<dim3(N / 4, all_fields ? 1 : 3, 1), dim3(NT1), LB1, st>>>(A1);
    k_or_pass2<N, P><<<dim3(N / 4, 2, 1), dim3(NT2), LB2, st>>>(A2);
    return hipGetLastError();
}

// OceanRenderer velocity of the current phase into d_vel [res^2][3], per second of delta_time: the weighted spectrum (first use / after a spectrum change), the
// passes, then the material's vertex stage (k_or_displace_mesh, the sampling mw_ocean_displace_mesh does) with unit_width = 0: (rate
// textures) / 8 at every vertex.  Single-ocean handles only (the caller checks).
static inline mw_status or_velocity(const OrState& s, VelState& v, int res, float* d_vel, hipStream_t st) {
    const size_t MM = (size_t)s.M * s.M;
    if (!v.disp) {  // the last buffer allocated: a failure half-way frees them all, and the next call starts again
#define VEL_ALLOC(ptr, bytes) if (hipMalloc((void**)&(ptr), (bytes)) != hipSuccess) { vel_free(v); return fail(MW_ENOMEM, "velocity: hipMalloc failed"); }
        VEL_ALLOC(v.initT, sizeof(f4) * MM) VEL_ALLOC(v.PQT, sizeof(f4) * MM) VEL_ALLOC(v.phase, sizeof(float) * MM)
        VEL_ALLOC(v.E, sizeof(cf) * 3 * MM) VEL_ALLOC(v.height, sizeof(float) * MM) VEL_ALLOC(v.disp_g, sizeof(float) * MM)
        VEL_ALLOC(v.disp, sizeof(cf) * MM)
#undef VEL_ALLOC
    }
    const unsigned nb = (unsigned)((MM + 255) / 256);
    if (!v.ready) {
        k_or_velocity_init<<<dim3(nb), dim3(256), 0, st>>>(s.M, s.omT, s.mult, s.initT, v.initT);
        k_or_prep<<<dim3(nb, 1), dim3(256), 0, st>>>(s.M, v.initT, v.PQT);
        if (hipGetLastError() != hipSuccess) return fail(MW_EDEVICE, "velocity spectrum launch failed");
        v.ready = true;
    }
    hipError_t e = hipSuccess;
    MW_FOR_SIZE(s.M, return fail(MW_EINVAL, "OceanRenderer: unsupported texture size"), e = or_velocity_passes<NN>(s, v, st));
    if (e != hipSuccess) return fail(MW_EDEVICE, std::string("velocity pass launch: ") + hipGetErrorString(e));
    const unsigned nv = (unsigned)res * (unsigned)res;
    // normals / whitecap are not sampled (NULL outputs): the texture arguments are never read
    k_or_displace_mesh<<<dim3((nv + 255) / 256, 1), dim3(256), 0, st>>>(s.M, res, 0.f, v.height, v.disp, v.height, v.height, d_vel, nullptr,
                                                                       nullptr);
    if (hipGetLastError() != hipSuccess) return fail(MW_EDEVICE, "velocity vertex stage launch failed");
    return MW_OK;
}
#endif

}  // namespace mw
