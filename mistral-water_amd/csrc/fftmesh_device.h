// fftmesh_device.h -- FFTMesh in the device build: the __global__ wrappers of the pass kernels (bodies: fftmesh_kernels.h), their launch forms
// over N, the host state FmState and the one path from a spectrum to a frame.  Included by mistral_water.hip alone, where its kernels stand.
#pragma once
// ------------------------------------------------------------------------------------------------
// __global__ wrappers: FFTMesh semantics
// ------------------------------------------------------------------------------------------------
__global__ void k_spectrum(int N, float length, float wind_x, float wind_y, float amplitude, float gravity,
                           uint64_t seed, cf* h0, cf* h0c) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * N) return;
    spectrum_element(N, length, wind_x, wind_y, amplitude, gravity, seed, idx / N, idx % N, h0, h0c);
}

__global__ void k_rest_mesh(int N, float unit_width, float* vertices, float* normals, float* uvs, int32_t* indices) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * N) return;
    rest_mesh_element(N, unit_width, idx / N, idx % N, vertices, normals, uvs, indices);
}

__global__ void k_prep(int N, float length, float gravity, const cf* h0, const cf* h0c, const cf* Wpre, f4* PQt,
                       f4* dPQ_i0, f4* dPQ_j0, float* Om) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * N) return;
    // idx enumerates the TRANSPOSED array so that the writes are the coalesced side
    prep_element(N, length, gravity, idx % N, idx / N, h0, h0c, Wpre, PQt, dPQ_i0, dPQ_j0, Om);
}

__global__ void k_omega_t(int N, float length, float gravity, float t, float* out) {
    int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= N * N) return;
    out[idx] = omega_t_f32(N, length, gravity, idx / N, idx % N, t);
}

#if defined(MW_TIMING) && !defined(MW_LAB)
#error "MW_TIMING (cycle stamps inside the pass kernels) is a lab build option: add -DMW_LAB (tools/build_variant.sh does)"
#endif
#ifdef MW_TIMING
#ifndef MW_STAMP_STEP
#define MW_STAMP_STEP 3
#endif
__device__ long long g_stamps[2][64][16][32];  // [kernel][block slot][wave][stamp]
#define MW_STAMP(K, id)                                                                               \
    do {                                                                                              \
        if ((blockIdx.x % 37) == 5 && blockIdx.x / 37 < 64 && step == MW_STAMP_STEP && (threadIdx.x & 63) == 0 && threadIdx.x < 1024) \
            g_stamps[K][blockIdx.x / 37][threadIdx.x >> 6][id] = __builtin_readcyclecounter();        \
    } while (0)
// the constant 100-MHz clock beside the cycle counter (slots 30 / 31: start / end of a kernel): calibrates cycles against kernel time
#define MW_STAMP_RT(K, id)                                                                            \
    do {                                                                                              \
        if ((blockIdx.x % 37) == 5 && blockIdx.x / 37 < 64 && step == MW_STAMP_STEP && (threadIdx.x & 63) == 0 && threadIdx.x < 1024) \
            g_stamps[K][blockIdx.x / 37][threadIdx.x >> 6][id] = __builtin_amdgcn_s_memrealtime();    \
    } while (0)
// where the 4-wave workgroups of a pass-1 launch ran: HW_ID / XCC_ID of EVERY workgroup b < 768, parked in the unused wave slots 4..15
#define MW_STAMP_HWID(K)                                                                              \
    do {                                                                                              \
        if (threadIdx.x == 0 && blockIdx.x < 768 && step == MW_STAMP_STEP) {                          \
            g_stamps[K][blockIdx.x % 64][4 + blockIdx.x / 64][0] = __builtin_amdgcn_s_getreg(63492);   \
            g_stamps[K][blockIdx.x % 64][4 + blockIdx.x / 64][1] = __builtin_amdgcn_s_getreg(63508);   \
            g_stamps[K][blockIdx.x % 64][4 + blockIdx.x / 64][2] = __builtin_amdgcn_s_memrealtime();    \
        }                                                                                             \
    } while (0)
#define MW_STAMP_HWID_END(K)                                                                          \
    do {                                                                                              \
        if (threadIdx.x == 0 && blockIdx.x < 768 && step == MW_STAMP_STEP)                            \
            g_stamps[K][blockIdx.x % 64][4 + blockIdx.x / 64][3] = __builtin_amdgcn_s_memrealtime();    \
    } while (0)
#elif defined(MW_SCHED_FENCE)
#define MW_STAMP(K, id) __builtin_amdgcn_sched_barrier(0)
#define MW_STAMP_RT(K, id) do { } while (0)
#define MW_STAMP_HWID(K) do { } while (0)
#define MW_STAMP_HWID_END(K) do { } while (0)
#else
#define MW_STAMP(K, id) do { } while (0)
#define MW_STAMP_RT(K, id) do { } while (0)
#define MW_STAMP_HWID(K) do { } while (0)
#define MW_STAMP_HWID_END(K) do { } while (0)
#endif

// LDS layout of both pass kernels: [twiddle tables, if small] [one set of exchange buffers]; a second (WAR) barrier follows
// every load.
// VT = virtual threads per lane (see k_pass2_hs): the phase functions are written for 4*T virtual threads (4 spectrum
// columns x T); a workgroup of 4*T/VT lanes runs virtual threads tid, tid + NT, ... of every phase back to back.
// issue priority (s_setprio, 0..3) of the row groups by field once the loads are out: the slope groups -- the longest fetch, then the
// normals to store -- ahead of displacement and halo row, the height groups (which only wait for hds after their transform) last.
// Measured on top of the wave-level exchanges: pass 2 of a lone step 17.1 -> 15.6 us (the reverse order 16.6; profiles/r04_ab_notes.md).
#ifndef MW_FRAME_PRIO_S
#define MW_FRAME_PRIO_S 3
#endif
#ifndef MW_FRAME_PRIO_D
#define MW_FRAME_PRIO_D 2
#endif
#ifndef MW_FRAME_PRIO_X
#define MW_FRAME_PRIO_X 2
#endif
#ifndef MW_FRAME_PRIO_H
#define MW_FRAME_PRIO_H 1
#endif
__device__ __forceinline__ void mw_setprio(int p) {  // the builtin wants a literal
    switch (p) {
        case 0: __builtin_amdgcn_s_setprio(0); break;
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        default: __builtin_amdgcn_s_setprio(3); break;
    }
}
// FS = the single-step (frame-at-a-time) instantiation: one FIELD per workgroup, a 1-D grid over A.jobs
template <int N, int P, int VT, bool FS = false>
__global__ __launch_bounds__((P1Geom<N, P>::NTHREADS / VT))
__attribute__((amdgpu_waves_per_eu(VT > 1 ? P1Geom<N, P>::NTHREADS / VT / 256 : (P == 8 ? MW_WAVES_P1 : 4)))) void k_pass1(P1Args A, StepTimes times) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using G = P1Geom<N, P>;
    cf* lds = reinterpret_cast<cf*>(smem);
    constexpr int T = FftGeom<N, P>::T, NT = G::NTHREADS / VT;
    static_assert(G::NTHREADS % VT == 0 && (VT == 1 || NT % T == 0), "a lane's virtual threads must belong to whole columns");
    const int tid = threadIdx.x;
    int jb = blockIdx.x, step = blockIdx.y;
    // Frame-at-a-time plan (A.field_split, single-step enqueues): one FIELD per workgroup instead of the three one after the
    // other, each workgroup re-forming the (cheap) animated spectrum.  A step is 257 workgroups at
    // 1024^2 where the device has 1024 slots, so its latency is that of ONE workgroup: a third of the work each cuts it
    // accordingly.  The arithmetic of a field does not depend on which workgroup runs it: same bits as the batched plan.
    int f_lo = 0, f_hi = 3;
    if constexpr (FS) {
        const int job = A.jobs[blockIdx.x];  // 1-D grid over the list of active (column job, field) pairs (p1_frame_jobs)
        if (job < 0) return;
        jb = job & 0xffff;
        f_lo = job >> 16;
        f_hi = f_lo + 1;
        step = 0;
        if (!p1_field_active(N, jb, f_lo, G::CW)) return;  // block-uniform, before any barrier
    } else if (A.tgroup > 0 && !p1_block_map((int)blockIdx.x, G::GRID_X, A.nsteps, A.tgroup, &jb, &step)) return;
    // Up to its last exchange a column's buffer is written and read by the column's own T threads: where those are one wave (the
    // single-step plan at T == 64) the exchanges need that wave's LDS operations in order and no workgroup barrier -- the four columns
    // drift apart; the last exchange feeds the column-interleaved final pass and keeps the barrier.
    constexpr bool WS = FS && VT == 1 && T == 64;
    auto col_sync = [&](bool whole_group) {
        if (WS && !whole_group) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
        else __syncthreads();
    };
    (void)col_sync;
    const float t = times.t[step];
    TwStage<N, P, NT> tws;
    if (TwGeom<N, P>::LDS_ALL) tws.load(A.TW, tid);  // in LDS behind the spectrum requests, visible after the first barrier
    const Twiddles tw = TwGeom<N, P>::view(A.TW, lds);
    cf* set0 = lds + G::TW_LDS;
    P1State<P> st[VT];
    cf x[VT][P];
#define MW_VT(h) for (int h = 0; h < VT; h++)
#define MW_BUF(h) (set0 + ((tid + (h) * NT) / T) * G::BUFSTRIDE)
#define MW_U(h) ((tid + (h) * NT) % T)
    MW_STAMP(0, 0);
    MW_STAMP_RT(0, 30);
    if constexpr (FS) MW_STAMP_HWID(0);
#pragma unroll
    MW_VT(h) p1_animate<N, P>(A, jb, tid + h * NT, t, st[h]);
    if (TwGeom<N, P>::LDS_ALL) tws.store(lds, tid);
    MW_STAMP(0, 1);
#pragma unroll
    for (int f = 0; f < 3; f++) {
        if (f < f_lo || f >= f_hi) continue;              // block-uniform: the frame-at-a-time plan runs one field per workgroup
        if (!p1_field_active(N, jb, f, G::CW)) continue;  // block-uniform: height needs columns j <= N/2 only
#pragma unroll
        MW_VT(h) p1_build<N, P>(A, jb, tid + h * NT, f, st[h], x[h]);
        if (f) __syncthreads();
        MW_STAMP(0, 2 + 8 * f);
#pragma unroll
        MW_VT(h) stage0_store<N, P, +1>(x[h], MW_U(h), MW_BUF(h));
        MW_STAMP(0, 3 + 8 * f);
        __syncthreads();  // the first barrier of the kernel also publishes the staged twiddle tables: always the whole group
#pragma unroll
        for (int s = 1; s < p1_mid_passes<N, P>(); s++) {
#pragma unroll
            MW_VT(h) load_slots<N, P>(x[h], MW_U(h), MW_BUF(h), s - 1);
            if (s == 1) MW_STAMP(0, 4 + 8 * f);
            col_sync(false);
            if (s == 1) MW_STAMP(0, 5 + 8 * f);
#pragma unroll
            MW_VT(h) stage_store<N, P, +1>(x[h], MW_U(h), MW_BUF(h), tw, s);
            if (s == 1) MW_STAMP(0, 6 + 8 * f);
            col_sync(s == p1_mid_passes<N, P>() - 1);
        }
        MW_STAMP(0, 7 + 8 * f);
#pragma unroll
        MW_VT(h) p1_finish<N, P>(A, tw, jb, step, tid + h * NT, f, x[h], set0);
        MW_STAMP(0, 8 + 8 * f);
    }
    MW_STAMP(0, 26);
    MW_STAMP_RT(0, 31);
    if constexpr (FS) MW_STAMP_HWID_END(0);
#undef MW_VT
#undef MW_BUF
#undef MW_U
}

#ifndef MW_XCD_GROUP
#define MW_XCD_GROUP 8  // adjacent row blocks kept on one XCD (1 = plain round-robin); 8-32: pass 2 -3 % at steady clocks
#endif
template <int NBLK>
__device__ __forceinline__ int p2_row_block(int b) {
    constexpr int XG = MW_XCD_GROUP;
    const int xcd = b % 8, cidx = b / 8;
    return (XG > 1 && NBLK % (8 * XG) == 0) ? (cidx / XG) * (8 * XG) + xcd * XG + (cidx % XG) : b;
}

template <int N, int P, int R2, bool DUMP = false>
__global__ __launch_bounds__((P2Geom<N, P, R2>::NTHREADS)) __attribute__((amdgpu_waves_per_eu(P == 8 ? MW_WAVES_P2 : 3))) void k_pass2(
    P2Args A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using G = P2Geom<N, P, R2>;
    cf* lds = reinterpret_cast<cf*>(smem);
    constexpr int T = FftGeom<N, P>::T;
    const int tid = threadIdx.x, step = blockIdx.y;
    // XCD-aware row-block mapping: the dispatcher places block b on XCD b % 8 (speed only, never correctness); giving
    // each XCD a contiguous range of row blocks makes a block's halo row (the first row of the NEXT block) a hit in
    // the same XCD's L2 instead of a second 128-B line fill across the fabric.
    const int ab = p2_row_block<N / R2>((int)blockIdx.x);
    const int g = tid / T;
    TwStage<N, P, G::NTHREADS> tws;
    if (TwGeom<N, P>::LDS_ALL) tws.load(A.TW, tid);
    const Twiddles tw = TwGeom<N, P>::view(A.TW, lds);
    cf* set0 = lds + G::TW_LDS;
    float* noise_lds = reinterpret_cast<float*>(lds + G::NOISE_OFF);
    P2State<P> st;
    cf x[P];
    MW_STAMP(1, 0);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int f = p2_field(k);
        const bool active = p2_active<N, P, R2>(ab, tid, f);
        if (k) __syncthreads();
        MW_STAMP(1, 1 + 8 * k);
        if (active) p2_load<N, P, R2>(A, ab, step, tid, f, x, set0);
        if (k == 0 && TwGeom<N, P>::LDS_ALL) tws.store(lds, tid);  // published by the barrier below
        MW_STAMP(1, 2 + 8 * k);
        __syncthreads();
#pragma unroll
        for (int s = 1; s < FftGeom<N, P>::S; s++) {
            const bool in_regs = LastStays<N, P>::value && s == FftGeom<N, P>::S - 1;  // the last pass writes nothing to LDS: no barrier on either side of it
            if (active) p2_mid_load<N, P, R2>(tid, s, x, set0);
            if (!in_regs) __syncthreads();
            if (active) p2_mid_store<N, P, R2>(tw, tid, s, x, set0);
            if (!in_regs) __syncthreads();
        }
        MW_STAMP(1, 6 + 8 * k);
        if (active) p2_finish<N, P, R2>(A, tw, ab, step, tid, f, x, st, set0, noise_lds);
        MW_STAMP(1, 7 + 8 * k);
    }
    __syncthreads();
    MW_STAMP(1, 25);
    if (p2_active<N, P, R2>(ab, tid, 1)) p2_publish_hds<N, P, R2>(tid, st, set0);
    __syncthreads();
    if constexpr (DUMP) p2_dump_hds<N, P, R2>(A, ab, step, tid, G::NTHREADS, set0);  // test hook
    MW_STAMP(1, 26);
    if (g < R2) p2_epilogue<N, P, R2>(A, ab, step, tid, st, set0, noise_lds);
    MW_STAMP(1, 27);
}

// Pass 2, sequential-halo variant (large N): R2 row groups, no halo group.  Height and displacement fields first; then
// the vertices leave, every row publishes hds, rows 0..R2-2 form 1 - J, group 0 transforms the halo row in buffer 0, row R2-1 follows;
// the slope field comes last and its final pass writes normals and whitecap together.
//
// VT = "virtual threads" per lane: the phase functions are written for R2*T virtual threads; a workgroup of R2*T/VT
// lanes runs virtual threads tid, tid + NT, ... of every phase back to back.  With VT = 2 a 4096-point, 4-row block is 8
// waves instead of 16: each lane owns 2 x 16 points, the register budget doubles to 256 (the 16-wave form spilled 29
// dwords = 14 B of scratch traffic per grid point at its 128), the two independent rows of a lane give the scheduler two
// instruction streams to interleave, and every barrier joins half as many waves.
// minimum waves per SIMD the register allocator must leave room for: as many workgroups per CU as the LDS admits (at most 2)
constexpr int hs_min_waves(int nthreads, int lds_bytes) {
    const int wgs = (2 * lds_bytes <= 160 * 1024) ? 2 : 1;
    const int w = nthreads / 64 * wgs / 4;
    return w < 1 ? 1 : (w > 8 ? 8 : w);
}
template <int N, int P, int R2, int VT, bool DUMP = false>
__global__ __launch_bounds__((P2Geom<N, P, R2, true>::NTHREADS / VT))
__attribute__((amdgpu_waves_per_eu(hs_min_waves(P2Geom<N, P, R2, true>::NTHREADS / VT, P2Geom<N, P, R2, true>::LDS_BYTES)))) void k_pass2_hs(P2Args A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using G = P2Geom<N, P, R2, true>;
    cf* lds = reinterpret_cast<cf*>(smem);
    constexpr int T = FftGeom<N, P>::T, NT = G::NTHREADS / VT;  // NT lanes, each running VT virtual threads
    static_assert(G::NTHREADS % VT == 0 && NT % T == 0, "a lane's virtual threads must belong to distinct whole row groups");
    static_assert(T % 64 == 0, "row groups must be whole waves: the row group of a lane is treated as wave-uniform (512^2 at 16 points fails parity)");
    const int tid0 = threadIdx.x, step = blockIdx.y;
    const int ab = p2_row_block<N / R2>((int)blockIdx.x);  // neighbouring row blocks (halo rows, shared 128-B lines) on one XCD
    const int g0 = wave_uniform<true>(tid0 / T);  // row group of virtual thread 0; virtual thread h is in group g0 + h * NT / T
    TwStage<N, P, NT> tws;
    if (TwGeom<N, P>::LDS_ALL) tws.load(A.TW, tid0);
    const Twiddles tw = TwGeom<N, P>::view(A.TW, lds);
    cf* set0 = lds + G::TW_LDS;
    P2StateHS<P> st[VT];
    cf x[VT][P];
    // The halo row's lines are the next row block's own lines: fetched while that block (same XCD, same phase) loads
    // them too, they are L2 hits; fetched two phases later they have left the L2 and cost a second 128-B fill per
    // 32-B piece (measured +6 B per grid point).  Needs 2P spare VGPRs across the displacement transform: VT >= 2.
    // Not at 4096^2, where it measured slower (profiles/r03_ab_notes.md).
    constexpr bool HALO_EARLY = N <= 2048 && VT >= 2;
    cf xh[HALO_EARLY ? P : 1];  // halo row data parked in registers across the displacement transform
    const int tid = tid0;  // MW_STAMP
    MW_STAMP(1, 0);
#define MW_VT(h) for (int h = 0; h < VT; h++)
#define MW_VTID(h) (tid0 + (h) * NT)
    constexpr bool SPARTS = P2SlopeParts<N, P>::value;
    constexpr bool KEEP = KeepT1<N, P>::value && P2SlopeParts<N, P>::value;
    cf t1m[KEEP ? VT : 1][KEEP ? P / 2 : 1];   // raw mirrored height-row values, from the height fetch to the slope assembly (KeepT1)
    (void)t1m;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int f = p2_hs_field(k);
        if (k != 0) __syncthreads();  // the previous phase's LDS reads are done (k = 0: nothing to wait for -- the twiddle tables
                                      // go to LDS behind the first requests below and are published by the barrier after stage 0)
        MW_STAMP(1, 1 + 8 * k);
        if (f == 2 && SPARTS) {  // the slope half of every virtual thread in flight, then height rows + stage 0 one at a time
#pragma unroll
            MW_VT(h) p2_fetch<N, P, R2, 1>(A, ab, step, MW_VTID(h), f, x[h]);
        } else {
#pragma unroll
            MW_VT(h) p2_fetch<N, P, R2>(A, ab, step, MW_VTID(h), f, x[h], (KEEP && f == 0) ? t1m[h] : nullptr);
        }
        if constexpr (HALO_EARLY)
            if (k == 1 && g0 == 0 && ab * R2 + R2 < N) p2_hs_halo_fetch<N, P, R2>(A, ab, step, tid0 % T, xh);
        if (k == 0 && TwGeom<N, P>::LDS_ALL) tws.store(lds, tid0);
        if (f == 2 && SPARTS) {
#pragma unroll
            MW_VT(h) {
                p2_fetch<N, P, R2, 2>(A, ab, step, MW_VTID(h), f, x[h], KEEP ? t1m[h] : nullptr);
                p2_stage0<N, P, R2>(MW_VTID(h), x[h], set0);
                mw_sched_fence();
            }
        } else {
#pragma unroll
            MW_VT(h) p2_stage0<N, P, R2>(MW_VTID(h), x[h], set0);
        }
        MW_STAMP(1, 2 + 8 * k);
        __syncthreads();
#pragma unroll
        for (int s = 1; s < FftGeom<N, P>::S; s++) {
            const bool in_regs = mw_pass_in_regs<N, P>(s);  // the last pass writes nothing to LDS (LastInRegs / LastInWave)
#pragma unroll
            MW_VT(h) p2_mid_load<N, P, R2>(MW_VTID(h), s, x[h], set0);
            if (!in_regs) __syncthreads();
#pragma unroll
            MW_VT(h) p2_mid_store<N, P, R2>(tw, MW_VTID(h), s, x[h], set0);
            if (!in_regs) __syncthreads();
        }
        MW_STAMP(1, 6 + 8 * k);
        if (f == 2) {
#pragma unroll
            MW_VT(h) p2_hs_finish_slopes<N, P, R2>(A, tw, ab, step, MW_VTID(h), x[h], st[h], set0);
            MW_STAMP(1, 7 + 8 * k);
            break;
        }
#pragma unroll
        MW_VT(h) p2_hs_finish<N, P, R2>(tw, ab, MW_VTID(h), f, x[h], st[h], set0);
        MW_STAMP(1, 7 + 8 * k);
        if (f != 1) continue;
        // ---- displacement done: vertices, halo row, Jacobian ----
#pragma unroll
        MW_VT(h) p2_vertices<N, P, R2>(A, ab, step, MW_VTID(h), st[h]);
        MW_STAMP(1, 24);
        __syncthreads();  // every final-pass read of the displacement buffers is done
#pragma unroll
        MW_VT(h) p2_publish_hds<N, P, R2>(MW_VTID(h), st[h], set0);  // every row into its own buffer, plain index b
        __syncthreads();
        if constexpr (DUMP) p2_dump_hds<N, P, R2>(A, ab, step, tid0, NT, set0);  // test hook
        const bool has_halo = (ab * R2 + R2 < N);  // block-uniform
        // Rows 0..R2-2 have their (a+1) neighbour published already: they form 1 - J now.  Buffer 0 (row 0's copy) is
        // then free for the halo row's transform; row R2-1 waits for it and works from its own published copy, so that
        // nobody's d is live across the halo transform (P = 16: the transform alone takes ~100 VGPRs).
#pragma unroll
        MW_VT(h) {
            const int g = g0 + h * (NT / T);
            if (g != R2 - 1) p2_hs_jacobian<N, P, R2>(ab, MW_VTID(h), st[h], set0 + g * G::BUFSTRIDE, set0 + (g + 1) * G::BUFSTRIDE);
        }
        __syncthreads();  // group 0 no longer reads its own row
        MW_STAMP(1, 25);
        if (has_halo) {  // group 0 = virtual thread 0 of the lanes below T
            const int u = tid0 % T;
            cf xq[P];  // the halo row in registers of its own: the allocator no longer ties it to x[0] (248 -> 219 VGPRs at 1024^2)
            if (g0 == 0) {
                if constexpr (HALO_EARLY) {
#pragma unroll
                    for (int q = 0; q < P; q++) xq[q] = xh[q];
                } else {
                    p2_hs_halo_fetch<N, P, R2>(A, ab, step, u, xq);
                }
                stage0_store<N, P, +1>(xq, u, set0);
            }
            __syncthreads();
#pragma unroll
            for (int s = 1; s < FftGeom<N, P>::S; s++) {
                const bool in_regs = mw_pass_in_regs<N, P>(s);
                if (g0 == 0) load_slots<N, P>(xq, u, set0, s - 1);
                if (!in_regs) __syncthreads();
                if (g0 == 0) { if (in_regs) stage_last_regs<N, P, +1>(xq, u, tw, s); else stage_store<N, P, +1>(xq, u, set0, tw, s); }  // g0 is wave-uniform: whole waves
                if (!in_regs) __syncthreads();
            }
            if (g0 == 0) {
                p2_last_load<N, P>(xq, u, set0);
                final_stage<N, P, +1>(xq, u, tw.TF);
            }
            __syncthreads();
            if (g0 == 0) p2_hs_halo_publish<N, P, R2>(ab, u, xq, set0);
            __syncthreads();
        }
        MW_STAMP(1, 26);
        if (g0 + (VT - 1) * (NT / T) == R2 - 1)  // the lane whose LAST virtual thread owns the block's last row
            p2_hs_jacobian_lds<N, P, R2>(ab, MW_VTID(VT - 1), st[VT - 1], set0 + (R2 - 1) * G::BUFSTRIDE, set0);
        MW_STAMP(1, 27);
    }
#undef MW_VT
#undef MW_VTID
}

// Pass 2 of a single-step enqueue (the frame-at-a-time plan, P2FrameGeom in fftmesh_kernels.h): 3 R2 + 1 row groups transform the
// three fields of the block's rows and the halo row at the same time; the latency of the workgroup -- which IS the latency of the
// step, 256 workgroups on 256 CUs -- is one transform instead of four.
template <int N, int P, int R2>
__global__ __launch_bounds__((P2FrameGeom<N, P, R2>::NTHREADS)) void k_pass2_frame(P2Args A) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using G = P2FrameGeom<N, P, R2>;
    static_assert(G::OK, "frame variant: geometry");
    cf* lds = reinterpret_cast<cf*>(smem);
    constexpr int T = G::T;
    const int tid = threadIdx.x, step = blockIdx.y;
    const int ab = p2_row_block<N / R2>((int)blockIdx.x);
    const int fg = wave_uniform<true>(tid / G::FT);  // 0 height, 1 displacement, 2 slopes, 3 the halo row (displacement of row a0 + R2)
    const int tl = tid - fg * G::FT;
    const bool has_halo = (ab * R2 + R2 < N);        // block-uniform
    const bool row = fg < 3, halo = (fg == 3) && has_halo;
    cf* set0 = lds + G::TW_LDS;
    cf* set_d = set0 + G::SETSTRIDE;
    cf* hbuf = set0 + 3 * G::SETSTRIDE;
    cf* mine = set0 + fg * G::SETSTRIDE;  // fg == 3: the halo row's buffer
    cf x[P];
    MW_STAMP(1, 0);
    MW_STAMP_RT(1, 30);
    TwStage<N, P, G::NTHREADS> tws;
    if (TwGeom<N, P>::LDS_ALL) tws.load(A.TW, tid);  // requested first (vmcnt is in order), written to LDS behind the row requests
    if (row) p2_fetch<N, P, R2>(A, ab, step, tl, fg, x);
    else if (halo) p2_hs_halo_fetch<N, P, R2>(A, ab, step, tl, x);
    if (TwGeom<N, P>::LDS_ALL) tws.store(lds, tid);
    const Twiddles tw = TwGeom<N, P>::view(A.TW, lds);
    if (row) p2_stage0<N, P, R2>(tl, x, mine);
    else if (halo) stage0_store<N, P, +1>(x, tl, mine);
    MW_STAMP(1, 1);
    __syncthreads();  // stage 0 was written in the row-interleaved mapping of the loads: every wave of a field into all of its rows
    // From here to the final pass a row buffer belongs to ONE wave (exact layouts: row-major mapping, T == 64): its exchanges need the
    // wave's own LDS operations in order, nothing else -- the row groups drift apart, and the first to finish starts its stores while
    // the others still transform.
    static_assert((T == 64 || T == 32) && G::FT % 64 == 0, "a wave holds whole row groups of one field");
    constexpr bool WSYNC = XLay<N, P>::EXACT;  // the middle passes of a row stay inside its own wave (the padded layouts' run row-interleaved: barriers)
    auto row_sync = [&]() {
        if constexpr (WSYNC) { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }
        else __syncthreads();
    };
    mw_setprio(fg == 0 ? MW_FRAME_PRIO_H : (fg == 1 ? MW_FRAME_PRIO_D : (fg == 2 ? MW_FRAME_PRIO_S : MW_FRAME_PRIO_X)));
#pragma unroll
    for (int s = 1; s < FftGeom<N, P>::S; s++) {
        const bool in_regs = mw_pass_in_regs<N, P>(s);
        if (row) p2_mid_load<N, P, R2>(tl, s, x, mine);
        else if (halo) load_slots<N, P>(x, tl, mine, s - 1);
        if (!in_regs) row_sync();
        if (row) p2_mid_store<N, P, R2>(tw, tl, s, x, mine);  // (fg is wave-uniform: the in-wave exchange of LastInWave runs in whole waves)
        else if (halo) { if (in_regs) stage_last_regs<N, P, +1>(x, tl, tw, s); else stage_store<N, P, +1>(x, tl, mine, tw, s); }
        if (!in_regs) row_sync();
    }
    MW_STAMP(1, 2);
    // the final pass reads a row buffer by its own row group alone, too: that group may write it again without a barrier
    cf* set_s = set0 + 2 * G::SETSTRIDE;
    if (row || halo) {
        p2_last_load<N, P>(x, tl % T, mine + (row ? tl / T : 0) * G::BUFSTRIDE);
        final_stage<N, P, +1>(x, tl % T, tw.TF);
    }
    MW_STAMP(1, 3);
    if (fg == 1) p2_frame_hds<N, P, R2>(ab, tl, x, set_d);
    else if (fg == 2) p2_frame_normals<N, P, R2>(A, ab, step, tl, x, set_s);
    else if (halo) p2_hs_halo_publish<N, P, R2>(ab, tl, x, hbuf);
    MW_STAMP(1, 4);
    __syncthreads();
    MW_STAMP(1, 5);
    if (fg == 0) p2_frame_vertices<N, P, R2>(A, ab, step, tl, x, set_d);
    else if (fg == 1) p2_frame_white<N, P, R2>(A, ab, step, tl, set_d, hbuf, set_s);
    MW_STAMP(1, 6);
    MW_STAMP_RT(1, 31);
}

// ---- kernel dispatch over N ----------------------------------------------------------------------
template <int N>
static hipError_t launch_pass1_n(const P1Args& A, const StepTimes& tm, int nsteps, hipStream_t st) {
    constexpr int P = Plan<N>::P1, VT = Plan<N>::VT1;
    static AttrOnce attr;  // per device: the attribute belongs to the function on the current device
    {
        hipError_t e = attr.set(reinterpret_cast<const void*>(&k_pass1<N, P, VT>), P1Geom<N, P>::LDS_BYTES);
        if (e != hipSuccess) return e;
    }
    constexpr int NT = P1Geom<N, P>::NTHREADS / VT, LB = P1Geom<N, P>::LDS_BYTES, GX = P1Geom<N, P>::GRID_X;
    if constexpr (mw_frame_plan_n(N)) {
        if (A.field_split) {
            static AttrOnce attrf;
            hipError_t e = attrf.set(reinterpret_cast<const void*>(&k_pass1<N, P, VT, true>), LB);
            if (e != hipSuccess) return e;
            k_pass1<N, P, VT, true><<<dim3(A.njobs), dim3(NT), LB, st>>>(A, tm);
            return hipGetLastError();
        }
    }
    if (A.tgroup > 0)
        k_pass1<N, P, VT><<<dim3(p1_grid_blocks(GX, nsteps, A.tgroup)), dim3(NT), LB, st>>>(A, tm);
    else
        k_pass1<N, P, VT><<<dim3(GX, nsteps), dim3(NT), LB, st>>>(A, tm);
    return hipGetLastError();
}
template <int N, bool DUMP>
static hipError_t launch_pass2_n(const P2Args& A, int nsteps, hipStream_t st) {
    constexpr int P = Plan<N>::P2, R2 = Plan<N>::R2;
    constexpr bool HS = Plan<N>::HS;
    constexpr int VT = HS ? Plan<N>::VT : 1;
    constexpr int NT = P2Geom<N, P, R2, HS>::NTHREADS / VT, LB = P2Geom<N, P, R2, HS>::LDS_BYTES;
    static AttrOnce attr;
    {
        const void* fn;
        if constexpr (HS) fn = reinterpret_cast<const void*>(&k_pass2_hs<N, P, R2, VT, DUMP>);
        else fn = reinterpret_cast<const void*>(&k_pass2<N, P, R2, DUMP>);
        hipError_t e = attr.set(fn, LB);
        if (e != hipSuccess) return e;
    }
    // Frame-at-a-time plan (FFTMesh.Update, S/FFTMesh.cs:60-73: ONE step per call; 256^2 to 1024^2): a step cannot fill the device,
    // its latency is that of one workgroup.  k_pass2_frame transforms the three fields of a row block side by side.  The arithmetic
    // of a row does not depend on which kernel runs it: same bits as the batched plan.
    if constexpr (mw_frame_plan_n(N) && !DUMP) {
        constexpr int RF = mw_frame_r2(N);
        if constexpr (P2FrameGeom<N, P, RF>::OK) {
            if (nsteps == 1) {
                static AttrOnce attrf;
                constexpr int LBF = P2FrameGeom<N, P, RF>::LDS_BYTES;
                hipError_t e = attrf.set(reinterpret_cast<const void*>(&k_pass2_frame<N, P, RF>), LBF);
                if (e != hipSuccess) return e;
                k_pass2_frame<N, P, RF><<<dim3(N / RF, 1), dim3(P2FrameGeom<N, P, RF>::NTHREADS), LBF, st>>>(A);
                return hipGetLastError();
            }
        }
    }
    if constexpr (HS)
        k_pass2_hs<N, P, R2, VT, DUMP><<<dim3(N / R2, nsteps), dim3(NT), LB, st>>>(A);
    else
        k_pass2<N, P, R2, DUMP><<<dim3(N / R2, nsteps), dim3(NT), LB, st>>>(A);
    return hipGetLastError();
}

// ---- host state: FmState, and the one path from a spectrum to a frame ------------------------------------------
// host-side geometry mirror of FftGeom<N,P> / Plan<N>
static int plan_points(int N, int pass) {
    MW_FOR_SIZE(N, return 16, return pass == 1 ? Plan<NN>::P1 : Plan<NN>::P2);
}
// the k_prep tables of sp from its (h0, h0c): the handle's spectrum at creation and after every change, the velocity's weighted one
static mw_status fm_prep(const FmSpectrum& sp, int N, float length, float gravity, const cf* Wpre, hipStream_t st) {
    hipLaunchKernelGGL(k_prep, dim3((N * N + 255) / 256), dim3(256), 0, st, N, length, gravity, sp.h0, sp.h0c, Wpre, sp.PQt, sp.dPQ_i0, sp.dPQ_j0, sp.Om);
    HIP_TRY(hipGetLastError());
    return MW_OK;
}

struct FmState {
    FmSpectrum sp;
    cf *TW = nullptr, *TW2 = nullptr, *Wpre = nullptr;  // twiddle tables of pass 1 / pass 2
    int* p1_jobs = nullptr; int p1_njobs = 0;  // single-step plan: pass-1 job list (p1_frame_jobs)
    int p1_tgroup = 8;  // time-steps of one pass-1 column job grouped on one XCD (p1_block_map): -25 % pass-1 time;
                        // switch MW_P1_TGROUP overrides (0 = plain 2-D grid)
    cf *E = nullptr, *Cj0 = nullptr; int e_cap = 0;  // the exchange buffers, and the steps they hold
    float *s_vert = nullptr, *s_norm = nullptr, *s_white = nullptr;  // 1-step scratch for the host API
    bool s_have = false;  // s_vert / s_norm / s_white hold a frame: the "latest frame" of mw_ocean_query_surface
    int s_wstride = 4;    // ... and the whitecap stride its writer used: 4 (RGBA colours, the host API) or 1 (the profiling hook)
    float s_t = 0.f, s_chop = 0.f;  // ... and the time and choppiness it was evaluated with (mw_ocean_velocity differentiates there)
};

// Every device buffer of an FmState besides its spectrum, named once: the rows fm_create allocates (and fills from `init`) and fm_free
// frees.  A row of 0 bytes is not creation's: the direct-sum path has no tables, the exchange buffers come with the first evaluation.
struct FmBuf { void** p; size_t bytes; const void* init; };
namespace { struct FmTables { std::vector<cf> tw, tw2, wpre; std::vector<int> jobs; }; }  // host copies of the FFT path's tables (empty: only freeing)
constexpr int FM_NBUF = 9;
static void fm_buffers(FmState& f, size_t NN, const FmTables& t, FmBuf (&b)[FM_NBUF]) {
    int n = 0;
    auto row = [&](auto*& p, size_t count, const void* init = nullptr) { b[n++] = FmBuf{(void**)&p, sizeof(*p) * count, init}; };
    row(f.s_vert, NN * 3); row(f.s_norm, NN * 3); row(f.s_white, NN * 4); row(f.E, 0); row(f.Cj0, 0);
    row(f.TW, t.tw.size(), t.tw.data()); row(f.TW2, t.tw2.size(), t.tw2.data()); row(f.Wpre, t.wpre.size(), t.wpre.data());
    row(f.p1_jobs, t.jobs.size(), t.jobs.data());
}
static void fm_free(FmState& f) {
    FmBuf b[FM_NBUF];
    fm_buffers(f, 0, FmTables(), b);
    for (const FmBuf& r : b) hipFree(*r.p);
    fm_spectrum_free(f.sp);
    f = FmState();
}
// The buffers of an N^2 grid, the twiddle tables [TS1 | TS2 | TS3 | TF] (TwGeom<N,P>) and the single-step job list of the FFT path, the
// initial spectrum of p and its prep tables; the launches go to st.  A failure leaves what it did allocate, for fm_free.
static mw_status fm_create(FmState& f, const mw_params& p, int N, bool use_fft, hipStream_t st) {
    const size_t NN = (size_t)N * N;
    FmTables t;
    if (use_fft) {
        t.tw = build_twiddle_table(N, plan_points(N, 1), +1);
        t.tw2 = build_twiddle_table(N, plan_points(N, 2), +1);
        t.wpre.resize(2 * N);
        for (int m = 0; m < 2 * N; m++) {
            double a = M_PI * (double)m / (double)N;  // (-1)^m e^{i pi m/N}
            double sg = (m & 1) ? -1.0 : 1.0;
            t.wpre[m] = mk((float)(sg * cos(a)), (float)(sg * sin(a)));
        }
        if (mw_frame_plan_n(N)) t.jobs = p1_frame_jobs(N, N >= MW_CW2_MIN_N ? 2 : 4);
    }
    f.p1_njobs = (int)t.jobs.size();
    mw_status s = fm_spectrum_alloc(f.sp, N, use_fft);
    if (s != MW_OK) return s;
    FmBuf b[FM_NBUF];
    fm_buffers(f, NN, t, b);
    for (const FmBuf& r : b) {
        if (r.bytes && (s = dmalloc(reinterpret_cast<char**>(r.p), r.bytes)) != MW_OK) return s;
        if (r.bytes && r.init) HIP_TRY(hipMemcpy(*r.p, r.init, r.bytes, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(k_spectrum, dim3((unsigned)((NN + 255) / 256)), dim3(256), 0, st, N, p.length, p.wind_x, p.wind_y, p.amplitude,
                       p.gravity, p.seed, f.sp.h0, f.sp.h0c);
    if (hipGetLastError() != hipSuccess) return fail(MW_EDEVICE, "k_spectrum launch failed");
    return use_fft ? fm_prep(f.sp, N, p.length, p.gravity, f.Wpre, st) : MW_OK;
}
// mw_ocean_reinit_spectrum on FFTMesh, transactional: the new spectrum is generated into buffers of its own and what is derived from it and
// from the length is rebuilt from there -- the prep tables (FFT path), the direct-sum tables d of the new length (otherwise; here and
// not inside the next enqueue).  The handle adopts the new buffers and frees the old ones only once every step has succeeded; otherwise
// it keeps the old spectrum and puts the tables of the old length p.length back.  No staging in `scratch`: another host entry point
// cannot clobber the new spectrum half-way.
static mw_status fm_reinit(FmState& f, DirectState& d, const mw_params& p, int N, bool use_fft, float length, float wind_x, float wind_y,
                           float amplitude, uint64_t seed, hipStream_t st) {
    const size_t NN = (size_t)N * N;
    cf *n0 = nullptr, *n0c = nullptr, *old0 = f.sp.h0, *old0c = f.sp.h0c;
    mw_status s = dmalloc(&n0, NN);
    if (s == MW_OK) s = dmalloc(&n0c, NN);
    if (s != MW_OK) { hipFree(n0); hipFree(n0c); return s; }
    auto tables = [&](float len) { return use_fft ? fm_prep(f.sp, N, len, p.gravity, f.Wpre, st) : direct_tables(d, N, p.unit_width, len, p.gravity, st); };
    hipLaunchKernelGGL(k_spectrum, dim3((unsigned)((NN + 255) / 256)), dim3(256), 0, st, N, length, wind_x, wind_y, amplitude, p.gravity, seed, n0, n0c);
    hipError_t e = hipGetLastError();
    f.sp.h0 = n0; f.sp.h0c = n0c;
    if (e == hipSuccess && use_fft) s = tables(length);
    if (e == hipSuccess && s == MW_OK) e = hipStreamSynchronize(st);
    if (e != hipSuccess) s = fail(MW_EDEVICE, std::string("mw_ocean_reinit_spectrum: ") + hipGetErrorString(e));
    if (s == MW_OK && !use_fft) s = tables(length);
    if (s == MW_OK) { hipFree(old0); hipFree(old0c); return MW_OK; }
    const std::string why = g_err;  // (the way back may fail() as well: if the device is gone, the handle is too)
    f.sp.h0 = old0; f.sp.h0c = old0c;
    (void)tables(p.length);
    (void)hipStreamSynchronize(st);
    hipFree(n0); hipFree(n0c);
    return fail(s, why);
}
// the exchange buffers hold nsteps steps afterwards; growing waits for the work on st that may still read the old ones
static mw_status ensure_exchange(FmState& f, int N, int nsteps, hipStream_t st) {
    if (f.e_cap >= nsteps) return MW_OK;
    if (f.E) {
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipFree(f.E));
        HIP_TRY(hipFree(f.Cj0));
        f.E = f.Cj0 = nullptr; f.e_cap = 0;
    }
    mw_status s = dmalloc(&f.E, (size_t)nsteps * 3 * N * N);
    if (s != MW_OK || (s = dmalloc(&f.Cj0, (size_t)nsteps * 3 * N)) != MW_OK) return s;
    f.e_cap = nsteps;
    return MW_OK;
}
// time-steps of one pass-1 column job issued back to back on one XCD (p1_block_map): the largest divisor of nsteps up to
// the handle's p1_tgroup (8), any divisor -- a 20-step enqueue groups by 5 --, 0 = plain 2-D grid
static int p1_time_group(const FmState& f, int nsteps) {
    for (int g = f.p1_tgroup; g > 1; g--)
        if (nsteps % g == 0) return g;
    return 0;
}
static mw_status launch_pass1(const FmState& f, const FmSpectrum& sp, const OceanConsts& c, const StepTimes& tm, int nsteps, hipStream_t st) {
    P1Args A;
    A.PQt = sp.PQt; A.dPQ_i0 = sp.dPQ_i0; A.dPQ_j0 = sp.dPQ_j0; A.Om = sp.Om; A.TW = f.TW;
    A.E = f.E; A.Cj0 = f.Cj0; A.c = c; A.nsteps = nsteps;
    A.tgroup = p1_time_group(f, nsteps);
    A.field_split = nsteps == 1 && mw_frame_plan_n(c.N);
    if (A.field_split) { A.jobs = f.p1_jobs; A.njobs = f.p1_njobs; }
    hipError_t e = hipSuccess;
    MW_FOR_SIZE(c.N, return fail(MW_EINVAL, "unsupported FFT size"), e = launch_pass1_n<NN>(A, tm, nsteps, st));
    if (e != hipSuccess) return fail(MW_EDEVICE, std::string("pass1 launch: ") + hipGetErrorString(e));
    return MW_OK;
}
template <bool DUMP>  // DUMP: pass 2 also stores hds at hds_dump (test hook)
static mw_status launch_pass2(const FmState& f, const OceanConsts& c, int nsteps, float* dv, float* dn, float* dw, int white_stride,
                              cf* hds_dump, hipStream_t st) {
    P2Args A;
    A.E = f.E; A.Cj0 = f.Cj0; A.TW = f.TW2; A.vertices = dv; A.normals = dn; A.white = dw; A.white_stride = white_stride;
    A.hds_dump = hds_dump; A.c = c;
    hipError_t e = hipSuccess;
    MW_FOR_SIZE(c.N, return fail(MW_EINVAL, "unsupported FFT size"), e = launch_pass2_n<NN, DUMP>(A, nsteps, st));
    if (e != hipSuccess) return fail(MW_EDEVICE, std::string("pass2 launch: ") + hipGetErrorString(e));
    return MW_OK;
}

// nsteps time-steps t[] of the spectrum sp into (dv, dn, dw) [nsteps][N*N][...], on st: the exchange buffers, pass 1, pass 2.  rest0: pass 2
// writes around a zero rest coordinate (unit_width = 0: the velocity).  hds_dump: pass 2 also stores hds there (test hook).  between:
// recorded on st between the two passes (profiling hook).
static mw_status fm_evaluate(FmState& f, const FmSpectrum& sp, OceanConsts c, const float* t, int nsteps, float* dv, float* dn, float* dw,
                             int white_stride, hipStream_t st, bool rest0 = false, cf* hds_dump = nullptr, hipEvent_t* between = nullptr) {
    mw_status s = ensure_exchange(f, c.N, nsteps, st);
    if (s != MW_OK) return s;
    StepTimes tm;
    for (int k = 0; k < nsteps; k++) tm.t[k] = t[k];
    if ((s = launch_pass1(f, sp, c, tm, nsteps, st)) != MW_OK) return s;
    if (between) hipEventRecord(*between, st);
    if (rest0) c.unit_width = 0.f;
    return hds_dump ? launch_pass2<true>(f, c, nsteps, dv, dn, dw, white_stride, hds_dump, st)
                    : launch_pass2<false>(f, c, nsteps, dv, dn, dw, white_stride, nullptr, st);
}
// the host-API frame (and hds of the same step, if asked for) to the arrays the caller gave, then wait for st
static mw_status fm_frame_to_host(const FmState& f, size_t NN, float* vertices_xyz, float* normals_xyz, float* colors_rgba, const cf* d_hds,
                                  float* hds_xy, hipStream_t st) {
    const struct { float* host; const void* dev; size_t floats; } part[4] = {{vertices_xyz, f.s_vert, 3}, {normals_xyz, f.s_norm, 3}, {colors_rgba, f.s_white, 4}, {hds_xy, d_hds, 2}};
    for (const auto& p : part)
        if (p.host) HIP_TRY(hipMemcpyAsync(p.host, p.dev, NN * p.floats * sizeof(float), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return MW_OK;
}
