/*
 * mistral_water.h -- C ABI of libmistral_water.so, the MI355X (gfx950) ocean heightfield synthesiser.
 *
 * The reference (AlphaMistral/Mistral-Water, a Unity C# project) has NO native plugin / P/Invoke
 * interface: the boundary is cut here at the seam between the MonoBehaviour drivers
 * and the private numerical methods they call on themselves.  Every entry point cites the reference
 * code it replaces (S/ = Assets/Mistral Water/Scripts/, F/ = .../Shaders/FFT/, W/ = .../Shaders/).
 *
 * Conventions
 *  - plain C, no C++ types, no callbacks; status codes only (never exceptions / aborts);
 *    mw_last_error() returns a thread-local description of the last failure.
 *  - arrays use the reference's layouts: Vector2 = 2 x f32, Vector3 = 3 x f32, Color = 4 x f32,
 *    grid index idx = i*N + j with i along x and j along z (S/FFTMesh.cs:110).
 *  - "host" entry points take host pointers and are synchronous (kernels + D2H done on return);
 *    "_device" entry points take device pointers, enqueue on the handle's stream and return at once.
 *  - one mw_ocean must not be used from two threads at once; distinct handles may be.
 *  - the library is HIP-only: there is NO CPU fallback.  mw_ocean_create fails with MW_EDEVICE when
 *    no gfx950 device is usable.
 */
#ifndef MISTRAL_WATER_H
#define MISTRAL_WATER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MW_ABI_VERSION 4

typedef struct mw_ocean mw_ocean; /* opaque; one per FFTMesh / OceanRenderer instance */

typedef enum {
    MW_OK = 0,
    MW_EINVAL = 1,           /* bad argument / NULL pointer / unsupported resolution */
    MW_ENOTPOW2 = 2,         /* OceanRenderer semantics needs a power-of-two texture size (S/OceanRenderer.cs:231) */
    MW_ENOTCOMMENSURATE = 3, /* mw_ocean_set_periodic: the grid does not repeat (creation never returns it: unit_width != length/N is
                                served by the direct-sum kernel instead) */
    MW_ENOMEM = 4,
    MW_EDEVICE = 5,          /* no usable HIP device / HIP runtime error */
    MW_ESTATE = 6            /* call order violation (e.g. evaluate before a spectrum exists) */
} mw_status;

typedef enum {
    MW_SEM_FFTMESH = 0,       /* S/FFTMesh.cs: centred k, quantised dispersion, closed-form time, spectral normals */
    MW_SEM_OCEANRENDERER = 1  /* S/OceanRenderer.cs + the F/ shaders: FFT-order k, capillary dispersion, iterated phase */
} mw_semantics;

/* Public Inspector fields of S/FFTMesh.cs:9-23 and S/OceanRenderer.cs:10-19, plus the constants the
 * reference hard-codes (gravity = G = 9.81f, S/FFTMesh.cs:52, F/FFTCommon.cginc:9). */
typedef struct {
    int32_t resolution; /* FFTMesh: grid is resolution^2.  OceanRenderer: textures are (8*resolution)^2 (S/OceanRenderer.cs:136) */
    float unit_width;   /* unitWidth */
    float length;       /* length */
    float wind_x, wind_y; /* wind */
    float amplitude;    /* amplitude (OceanRenderer divides by 10000 itself, S/OceanRenderer.cs:149) */
    float choppiness;   /* choppiness */
    float gravity;      /* 9.81f in the reference */
    float t_division;   /* FFTMesh.tDivision  (S/FFTMesh.cs:70) */
    float mult;         /* OceanRenderer.mult (S/OceanRenderer.cs:223) */
    uint64_t seed;      /* seed of the library's documented counter RNG (the reference never seeds Unity's) */
    int32_t semantics;  /* mw_semantics */
    int32_t device;     /* HIP device ordinal */
} mw_params;

/* flags of mw_ocean_evaluate_device */
#define MW_OUT_WHITE_SCALAR 0u /* whitecap written as 1 float per vertex (the canonical 28 B/point output) */
#define MW_OUT_COLOR_RGBA 1u   /* whitecap replicated into a Unity Color (S/FFTMesh.cs:274), 16 B per vertex */

int32_t mw_abi_version(void);
/* Identity of this build of the library: "<16 hex digits of a hash over the kernel sources and compile flags> <flags tag>".
 * bench.py prints it and the committed rocprofv3 PMC summaries carry it, so a counter file is only ever quoted next to
 * numbers of the build it was measured on.                                                                          */
const char* mw_build_id(void);
const char* mw_last_error(void);
int32_t mw_device_count(void);
void mw_params_default(mw_params* p, int32_t semantics); /* Inspector defaults of the two MonoBehaviours */

/* ---- lifecycle --------------------------------------------------------------------------------
 * mw_ocean_create = SetParams + GenerateMesh's spectrum fill (S/FFTMesh.cs:90-99,114-116;
 * S/OceanRenderer.cs:116-170,209-214): allocates device state and generates h0 / h0conj on the GPU
 * from params->seed (Phillips, S/FFTMesh.cs:149-166; Box-Muller htilde0, :168-176).                */
mw_status mw_ocean_create(const mw_params* params, mw_ocean** out);
void mw_ocean_destroy(mw_ocean* o);
/* OceanRenderer semantics, `ntiles` independent oceans in ONE handle: tile k is the ocean of `params` with seed
 * params->seed + k.  One 1024^2 frame is three launches of a few hundred workgroups -- latency-, not bandwidth-bound -- and
 * the stateful phase (F/FFTCommon.cginc:101-104) forbids batching in time, so the tile axis is what fills the device: every
 * GenerateTexture() of the handle advances all tiles in the same three launches.  Every OceanRenderer entry point of a
 * batched handle takes / returns arrays with a leading tile axis ([ntiles][M*M*...], [ntiles][resolution^2*...] for
 * mw_ocean_displace_mesh); the rest mesh is one mesh.  Per-tile results are identical to single handles of seed + k.     */
mw_status mw_ocean_create_batch(const mw_params* params, int32_t ntiles, mw_ocean** out);
int32_t mw_ocean_batch_size(const mw_ocean* o);

/* Run all subsequent work of this handle on an existing hipStream_t (e.g. torch's current stream).  The argument means
 * what it says: NULL is HIP's legacy default stream (what torch.cuda.current_stream().cuda_stream is by default), as in
 * the pond entry points.  A fresh handle runs on its own private non-blocking stream; mw_ocean_use_own_stream returns to
 * it.  Work already enqueued on the previous stream is waited for before the switch.
 * LIFETIME CONTRACT: the stream belongs to the caller and must outlive its use by the handle -- call
 * mw_ocean_use_own_stream (or mw_ocean_set_stream with another stream, or mw_ocean_destroy) BEFORE destroying it.  A
 * destroyed hipStream_t is a dangling pointer to HIP; the library tolerates the error codes the runtime returns for one
 * ("nothing pending") as a courtesy, but cannot make the use of a freed handle defined.                              */
mw_status mw_ocean_set_stream(mw_ocean* o, void* hip_stream);
mw_status mw_ocean_use_own_stream(mw_ocean* o);
void* mw_ocean_get_stream(mw_ocean* o);
mw_status mw_ocean_synchronize(mw_ocean* o);

/* choppiness / tDivision / mult may change between frames without regenerating the spectrum
 * (S/FFTMesh.cs:244-245 reads choppiness every frame; S/OceanRenderer.cs:96).                      */
mw_status mw_ocean_set_choppiness(mw_ocean* o, float choppiness);

/* ---- the periodic surface: the surface services on the infinite tiling of the frame ---------------------------------
 * An FFTMesh frame on a grid that repeats -- unit_width * (float)N == length in float32 and N even, the chirp-z grids among them
 * (N = 100, unit_width 1, length 100) -- is periodic with period P = (float)N * unit_width (one float32 multiply).  With the switch
 * on, mw_ocean_query_surface, mw_ocean_query_velocity, mw_ocean_hull_forces and mw_ocean_step_bodies (host and device forms, both
 * plans of the bodies) read that tiling instead of the one footprint.  Off by default; with it off every call returns the bits it
 * always returned.  The switch is not part of the frame record: it needs no new frame and changes no output of mw_ocean_evaluate,
 * mw_ocean_update or mw_ocean_velocity.
 *   set_periodic(o, 1): MW_ENOTCOMMENSURATE on any other FFTMesh grid (the shipped N = 12, length 12.39 scene; an odd N, whose
 *     sum is ANTI-periodic); MW_ESTATE on an OceanRenderer handle -- its mesh samples clamp-addressed textures half a texel inside
 *     each edge, so vertex res-1 is not the image of vertex 0 and the mesh does not tile; MW_EINVAL on a batched handle, a NULL
 *     handle, or `on` outside {0, 1}.  set_periodic(o, 0) is always allowed.
 *   mw_ocean_reinit_spectrum to a length that breaks the condition turns the switch off.
 *   get_periodic: the switch and P (either out-argument may be NULL); P is reported whether or not the switch is on, 0 where the
 *     grid does not repeat.
 * The tiled surface:
 *   integer grid line g = k*N + a (floor division, 0 <= a < N) rests at rest(g) = rest_coord(a) + (float)k * P; for k = 0 this is
 *     exactly the rest coordinate of mw_ocean_rest_mesh;
 *   vertex (gi, gj) is vertex (ai, aj) of the frame displaced by (ki*P, 0, kj*P); its normal, whitecap and velocity are those of
 *     (ai, aj);
 *   every integer cell (gi, gj) exists and is split along the same diagonal; cell a = N-1, between the last grid line of a tile and
 *     the first of the next, is the seam (it is in no index buffer).
 *   Reduction first: a query (x, z) is reduced to (x', z') = (x - kx*P, z - kz*P) with x', z' in [rest(0), rest(0) + P], answered
 *     in the frame of the base tile (where the neighbouring tiles sit at +-P, +-2P, ...), and kx*P, kz*P are added to px and pz
 *     once, at the end.  The answer is a function of (x', z', kx, kz): its precision does not degrade with the distance from the
 *     origin.  The residual is computed in the base frame.
 *   MW_QUERY_REST: every finite point has an answer (no NaN off the footprint); a point inside the base footprint returns the same
 *     8 floats, bit for bit, as with the switch off.
 *   MW_QUERY_WORLD: the same walk (preconditioned step, 4-cell cap, in-triangle tolerance, best-so-far rule) but unclamped: it
 *     crosses seams and tile boundaries freely.  Where the non-periodic walk never touches its clamp the periodic one returns the
 *     same bits; folds still return the visited point of smallest residual.
 *   Non-finite points, and points whose tile index exceeds 2^20 in magnitude, give NaN in every field (status MW_OK).
 *   Hull vertices are located one by one, so a hull may straddle a seam; only eta, u and the residual come from the located point.
 *   Arithmetic: the tiled services run in strict float32 (no fused multiply-adds), so a g++ build of the same functions equals them
 *     bit for bit, as it does the raycasts; the one-footprint services keep the contracted arithmetic their bits have always come
 *     from.  The two "same bits" statements above hold between the two forms under one arithmetic; on the device a periodic answer
 *     inside the base footprint agrees with the switch-off answer to rounding, not bit for bit.
 * mw_ocean_raycast on a handle with the switch on returns MW_ESTATE: it reads the one footprint and does not tile.  The tiled surface
 *   has a cast of its own, mw_ocean_raycast_tiled (below), which does not read the switch.                                       */
mw_status mw_ocean_set_periodic(mw_ocean* o, int32_t on);                     /* 0 / 1 */
mw_status mw_ocean_get_periodic(mw_ocean* o, int32_t* on, float* period);     /* either out-argument may be NULL */

/* Inject / read back verttilde and vertConj (S/FFTMesh.cs:35-36,114-116), N*N*2 floats each,
 * idx = i*N + j.  Injection is how a caller reproduces a Unity-generated spectrum exactly, and
 * how the parity tests feed identical inputs to the oracle and to the GPU.                         */
/* OceanRenderer semantics: the same pair is initialTexture.rg / .ba (F/InitialSpectrum.shader:53), M*M*2 floats
 * each with texel (px,py) at index py*M + px; setting it restarts the phase at 0.                              */
mw_status mw_ocean_set_spectrum(mw_ocean* o, const float* h0_xy, const float* h0conj_xy);
mw_status mw_ocean_get_spectrum(mw_ocean* o, float* h0_xy, float* h0conj_xy);

/* Regenerate the initial spectrum IN PLACE from new (length, wind, amplitude, seed); everything else of the handle stays.
 *  OceanRenderer semantics = the parameter-change branch of Update (S/OceanRenderer.cs:98-109): RenderInitial() draws
 *    initialTexture again (pass the handle's own seed: the reference keeps _RandomSeed1/2); the stateful phase textures are
 *    NOT touched, so the animation continues; dispersion and spectrum passes use the new length from the next frame on
 *    (:94-97), while the normal pass keeps the length it was created with -- the reference sets normalMat's _Length only in
 *    SetParams (:163) and never again.
 *  FFTMesh semantics = the spectrum fill of GenerateMesh (S/FFTMesh.cs:114-116) with a new seed (the `generate` tick
 *    draws fresh UnityEngine.Random values, :62-68); the timer is not touched (mw_ocean_reset_timer does that).  The grid
 *    must stay on the same evaluation path: MW_ESTATE if the new length flips unit_width == length / N.
 *  The call is synchronous and transactional: the new spectrum is generated into buffers of its own (the handle transiently holds
 *  two spectra: 2 x N^2 x 8 B more, 268 MB at 4096^2), the derived tables -- and for non-FFT grids the chirp tables of the new
 *  length -- are rebuilt, the stream is drained, and only then are the old buffers freed (hipFree: a device-wide synchronisation).  */
mw_status mw_ocean_reinit_spectrum(mw_ocean* o, float length, float wind_x, float wind_y, float amplitude, uint64_t seed);

/* Save / restore the animation state.  OceanRenderer: the current phase texture (F/Dispersion.shader:32-41), M*M floats,
 * texel (px,py) at py*M + px -- with initialTexture (mw_ocean_get_spectrum) this is everything a checkpoint needs.
 * FFTMesh: the timer (mw_ocean_timer / mw_ocean_set_timer); get/set_phase return MW_ESTATE there.                    */
mw_status mw_ocean_get_phase(mw_ocean* o, float* phase);
mw_status mw_ocean_set_phase(mw_ocean* o, const float* phase);
mw_status mw_ocean_set_timer(mw_ocean* o, float timer);
/* OceanRenderer: the length the normal pass divides by.  The reference sets normalMat._Length once in SetParams
 * (S/OceanRenderer.cs:163) and never again, so after mw_ocean_reinit_spectrum with a new length it differs from the
 * handle's length.  It is the third piece of an OceanRenderer checkpoint (with initialTexture and the phase): a fresh
 * handle created with the current length must be given the saved value.  FFTMesh handles return their length and
 * refuse the setter with MW_ESTATE.                                                                              */
float mw_ocean_normal_length(const mw_ocean* o);
mw_status mw_ocean_set_normal_length(mw_ocean* o, float normal_length);

/* GenerateMesh outputs (S/FFTMesh.cs:101-139, S/OceanRenderer.cs:172-207): rest vertices [N*N*3],
 * normals [N*N*3], uvs [N*N*2], triangle indices [(N-1)^2*6].  Any pointer may be NULL.            */
mw_status mw_ocean_rest_mesh(mw_ocean* o, float* vertices_xyz, float* normals_xyz, float* uvs_xy, int32_t* indices);
int64_t mw_ocean_index_count(const mw_ocean* o);
int32_t mw_ocean_grid_size(const mw_ocean* o); /* N of the synthesis grid (8*resolution in OceanRenderer mode) */

/* ---- per-frame: FFTMesh.EvaluateWaves(t)  (S/FFTMesh.cs:224-280) -------------------------------
 * host outputs: mesh.vertices [N*N*3], mesh.normals [N*N*3], mesh.colors [N*N*4].                  */
mw_status mw_ocean_evaluate(mw_ocean* o, float t, float* vertices_xyz, float* normals_xyz, float* colors_rgba);

/* FFTMesh.Update (S/FFTMesh.cs:60-73): timer += delta_time / tDivision; EvaluateWaves(timer).      */
mw_status mw_ocean_update(mw_ocean* o, float delta_time, float* vertices_xyz, float* normals_xyz, float* colors_rgba);
float mw_ocean_timer(const mw_ocean* o);
mw_status mw_ocean_reset_timer(mw_ocean* o); /* the `generate` tick of S/FFTMesh.cs:62-68 */

/* Throughput form: nsteps independent time-steps t[0..nsteps) of the same ocean in one enqueue
 * (FFTMesh semantics is a pure function of (h0, h0conj, t), S/FFTMesh.cs:178-190).  Outputs stay in
 * device memory: d_vertices [nsteps][N*N*3], d_normals [nsteps][N*N*3], d_white [nsteps][N*N] or
 * [nsteps][N*N*4] with MW_OUT_COLOR_RGBA.  t is a HOST array.  Asynchronous on the handle's stream. */
mw_status mw_ocean_evaluate_device(mw_ocean* o, const float* t, int32_t nsteps, void* d_vertices, void* d_normals,
                                   void* d_white, uint32_t flags);
int32_t mw_ocean_max_batch(const mw_ocean* o); /* largest nsteps one enqueue accepts */

/* ---- per-frame: OceanRenderer.GenerateTexture()  (S/OceanRenderer.cs:216-316) ------------------
 * advances the stateful phase by delta_time*mult and produces the four result textures, host side:
 * height [M*M] (= heightTexture.r), disp_xz [M*M*2] (= displacementTexture.rb),
 * normal_xyz [M*M*3] (= normalTexture.rgb), white [M*M] (= whiteTexture.r); M = 8*resolution,
 * texel (px,py) at index py*M + px.  Any pointer may be NULL.
 * Plan: these four planar textures need only Re h, Re / Im Dx and Re Dz, so the planar entry points run TWO complex transforms per frame
 * (height + i Dz share one, built from the Hermitian parts of the initial spectrum: csrc/ocean_renderer_kernels.h) where the shaders
 * run three; the RGBA forms below, whose channels include Im h and Im Dz, run three.  Both are within the stated float32 tolerance of
 * the reference's pipeline; one frame through the two forms may differ in the last bits.  A phase texture injected with
 * mw_ocean_set_phase that is not mirror-symmetric (every phase the library produced is) selects three transforms here too.        */
mw_status mw_ocean_generate_texture(mw_ocean* o, float delta_time, float* height, float* disp_xz, float* normal_xyz,
                                    float* white);
mw_status mw_ocean_generate_texture_device(mw_ocean* o, float delta_time, void* d_height, void* d_disp_xz,
                                           void* d_normal_xyz, void* d_white);

/* Throughput form: nframes CONSECUTIVE GenerateTexture() calls of one ocean in one enqueue.  Frame k advances the stateful phase by
 * delta_time[k]*mult on top of frame k-1 (F/Dispersion.shader:32-41, F/FFTCommon.cginc:101-104) -- a per-texel chain of one multiply,
 * one add and one fmod that the spectrum kernel walks in registers -- while the three transforms and the normal / whitecap passes of
 * different frames are independent and run as nframes-deep launches (S/OceanRenderer.cs:216-307 per frame).  Results, the phase
 * included, are bit-identical to nframes calls of mw_ocean_generate_texture_device.  delta_time is a HOST array; device destinations
 * are d_height [nframes][M*M], d_disp_xz [nframes][M*M*2], d_normal_xyz [nframes][M*M*3], d_white [nframes][M*M]; a NULL destination
 * keeps that texture's frames in the handle (mw_ocean_frame_textures).  Afterwards the handle's latest frame (mw_ocean_displace_mesh,
 * mw_ocean_get_phase) is frame nframes-1.  1 <= nframes <= mw_ocean_max_frames; single-ocean handles only (a handle of
 * mw_ocean_create_batch fills the device with tiles instead: MW_ESTATE).  Asynchronous on the handle's stream.                        */
mw_status mw_ocean_generate_texture_steps_device(mw_ocean* o, const float* delta_time, int32_t nframes, void* d_height,
                                                 void* d_disp_xz, void* d_normal_xyz, void* d_white);
/* The phase texture after nframes MORE GenerateTexture() calls with these delta times, without producing textures (the Dispersion pass alone,
 * F/Dispersion.shader:32-41; any nframes >= 0; delta_time is a HOST array): the handle then continues bit for bit like one that rendered
 * those frames.  How a rank of a multi-GPU job seeks to its own block of a frame sequence, and how a recorder skips frames.  Asynchronous.  */
mw_status mw_ocean_advance_phase(mw_ocean* o, const float* delta_time, int32_t nframes);
/* host form: the same nframes frames into host arrays [nframes][M*M*...] (any may be NULL); synchronous, PCIe-bound (28 B per texel and frame) */
mw_status mw_ocean_generate_texture_steps(mw_ocean* o, const float* delta_time, int32_t nframes, float* height, float* disp_xz,
                                          float* normal_xyz, float* white);
int32_t mw_ocean_max_frames(const mw_ocean* o); /* largest nframes one enqueue accepts (0: not an OceanRenderer handle) */
/* device pointers of frame `frame` of the LATEST steps call for the textures that call kept in the handle (NULL destination there);
 * a texture that went to a caller buffer reports NULL.  Valid until the next steps call of this handle.                              */
mw_status mw_ocean_frame_textures(mw_ocean* o, int32_t frame, void** d_height, void** d_disp_xz, void** d_normal_xyz, void** d_white);

/* ---- optional: page-lock caller arrays --------------------------------------------------------------------
 * The host-pointer entry points copy results into caller memory; into ordinary (pageable) arrays that copy runs at
 * ~9 GB/s and dominates the call.  A host that keeps its output arrays for many frames -- the
 * reference does: vertMeow/normals are allocated once (S/FFTMesh.cs:90-99) -- can register them once (in C#: after
 * GCHandle.Alloc(array, GCHandleType.Pinned)) and every later copy into them goes at PCIe rate.  Unregister before
 * the memory is freed or unpinned.                                                                               */
mw_status mw_host_register(void* ptr, size_t bytes);
mw_status mw_host_unregister(void* ptr);

/* ---- OceanRenderer semantics, consumer-side packing ---------------------------------------------------------
 * One GenerateTexture() delivered as the reference's four ARGBFloat render targets (S/OceanRenderer.cs:143-146,
 * bound to the ocean material at :310-313), [M*M*4] floats each, texel (px,py) at (py*M + px)*4:
 *   height_rgba = (Re h, Im h, Re h, Im h)      F/SpectrumHeight.shader:46 + F/Stockham.shader:56
 *   disp_rgba   = (Re Dx, Im Dx, Re Dz, Im Dz)  F/Spectrum.shader:50      + F/Stockham.shader:56
 *   normal_rgba = (n.x, n.y, n.z, 1)            F/OceanNormal.shader:55
 *   white_rgba  = (w, w, w, 1)                  F/WhiteCap.shader:44
 * Any destination may be NULL.  Host form synchronous, device form asynchronous on the handle's stream.          */
mw_status mw_ocean_generate_texture_rgba(mw_ocean* o, float delta_time, float* height_rgba, float* disp_rgba,
                                         float* normal_rgba, float* white_rgba);
mw_status mw_ocean_generate_texture_rgba_device(mw_ocean* o, float delta_time, void* d_height_rgba, void* d_disp_rgba,
                                                void* d_normal_rgba, void* d_white_rgba);
/* nframes consecutive frames (mw_ocean_generate_texture_steps_device) as the four ARGBFloat targets, [nframes][M*M*4] each.          */
mw_status mw_ocean_generate_texture_steps_rgba_device(mw_ocean* o, const float* delta_time, int32_t nframes, void* d_height_rgba,
                                                      void* d_disp_rgba, void* d_normal_rgba, void* d_white_rgba);
mw_status mw_ocean_generate_texture_steps_rgba(mw_ocean* o, const float* delta_time, int32_t nframes, float* height_rgba, float* disp_rgba,
                                               float* normal_rgba, float* white_rgba); /* host arrays [nframes][M*M*4], synchronous */
/* The ocean material's vertex stage on the resolution x resolution mesh of S/OceanRenderer.cs:172-207, sampling the
 * textures of the LATEST GenerateTexture() bilinearly at the vertex uv (tex2Dlod, clamp):
 *   vertex = rest + (_Anim.r, _Height.r, _Anim.b) / 8      W/TestOcean.shader:65-66, W/MistralWaterCommon.cginc:22-23
 *   normal = normalize(_Bump.rgb)                          W/TestOcean.shader:70
 *   color  = _White.r   (1 float per vertex)               W/TestOcean.shader:72, W/MistralWaterCommon.cginc:56
 * normals/colors may be NULL.  MW_ESTATE before the first GenerateTexture().                                      */
mw_status mw_ocean_displace_mesh(mw_ocean* o, float* vertices_xyz, float* normals_xyz, float* colors);
mw_status mw_ocean_displace_mesh_device(mw_ocean* o, void* d_vertices_xyz, void* d_normals_xyz, void* d_colors);

/* ---- surface queries: how high is the water here? ---------------------------------------------------------------
 * The surface of a frame is the displaced triangle mesh the library hands out:
 *   vertices  FFTMesh: what the latest mw_ocean_evaluate / mw_ocean_update returned (vertices, normals, colour R);
 *             OceanRenderer: what mw_ocean_displace_mesh returns for the selected frame (resolution^2 vertices);
 *   triangles the index buffer of mw_ocean_rest_mesh (S/FFTMesh.cs:101-139, S/OceanRenderer.cs:172-207): rest-grid cell (i, j)
 *             is split along its (i, j+1)-(i+1, j) diagonal;
 *   inside a triangle position, normal and whitecap are interpolated barycentrically in REST-plane coordinates; the normal
 *             is normalised afterwards.
 * A query is a horizontal point (x, z) in the object space of the vertex outputs; out is [n][8] floats per point:
 *   px, py, pz, nx, ny, nz, white, residual.
 *   MW_QUERY_REST:  (x, z) is a rest-plane position; the result is the displaced surface point the mesh carries there.
 *                   Rest positions outside the mesh footprint give NaN in every field (the status is still MW_OK).  residual = 0.
 *   MW_QUERY_WORLD: (x, z) is a position on the DISPLACED surface (buoyancy).  The rest point u with displaced(u).xz = (x, z) is
 *                   found by the iteration u <- (x, z) - D(u), D the horizontal displacement; the map is affine within a triangle,
 *                   so at every visited point one exact 2 x 2 solve in its triangle finishes the job when its solution lies inside
 *                   that triangle.  Otherwise the step is preconditioned by the inverse of the triangle's map (a Newton step of the
 *                   piecewise-affine map, at most 4 cells; the plain step in folded triangles), which keeps converging near the
 *                   fold limit where the plain iteration stalls.  `iterations` bounds the walk: 0 = the default, 8; at most 64.
 *                   residual = |displaced(u*).xz - (x, z)|: ~0 where the answer was found; where the mesh folds over itself
 *                   (strong choppiness: no unique answer) or (x, z) is off the displaced footprint, the visited point of smallest
 *                   residual is returned -- a point on the mesh -- with that residual.  Non-finite (x, z) give NaN.
 * frame: -1 = the latest frame (FFTMesh: latest mw_ocean_evaluate / update; OceanRenderer: what mw_ocean_displace_mesh samples);
 *        0..k-1 = frame of the latest OceanRenderer steps call, as mw_ocean_frame_textures (its textures must have stayed in the handle).
 * MW_ESTATE before the first frame; MW_EINVAL for a NULL array with n > 0, n < 0 or n > 2^32 - 256 (one launch), a bad mode,
 * iterations outside [0,64], a frame out of range, frame != -1 on an FFTMesh handle, or a batched handle (mw_ocean_create_batch).
 * n == 0 does nothing.  The query reads the frame and changes nothing of the handle's state.  OceanRenderer queries first run the
 * vertex stage of the frame into a buffer of the handle, reused by the next query in the order of the handle's stream (as every
 * entry point's staging is); mw_ocean_set_stream drains the previous stream before a switch, so queries on either side of a
 * switch cannot overlap.                                                                                                    */
#define MW_QUERY_REST 0
#define MW_QUERY_WORLD 1
/* xz [n][2], out [n][8]: host arrays, synchronous */
mw_status mw_ocean_query_surface(mw_ocean* o, int32_t frame, int32_t mode, const float* xz, int64_t n, int32_t iterations,
                                 float* out);
/* device arrays (d_xz 8-byte, d_out 16-byte aligned), asynchronous on the handle's stream */
mw_status mw_ocean_query_surface_device(mw_ocean* o, int32_t frame, int32_t mode, const void* d_xz, int64_t n,
                                        int32_t iterations, void* d_out);

/* ---- surface velocity: how fast does the water move here? -------------------------------------------------------
 * The time derivative of the vertices mw_ocean_query_surface reads, computed exactly from the spectrum (every output is linear in
 * it, and d/dt of h0 e^{iwt} + h0c e^{-iwt} is the same sum over (i w h0, -i w h0c)), not by differencing two frames:
 *   FFTMesh        velocity = (-choppiness dDx/dt, dh/dt, -choppiness dDz/dt) of vertex (x - chop Dx, h, z - chop Dz) at the t and
 *                  choppiness of the latest mw_ocean_evaluate / mw_ocean_update frame (or of the profiling hook's frame).  UNITS: per
 *                  unit of the time argument t.  mw_ocean_update advances t by delta_time / t_division, so the velocity per second
 *                  of delta_time is this value / t_division.  frame must be -1.
 *   OceanRenderer  velocity = d/dt of rest + (_Anim.r, _Height.r, _Anim.b) / 8, the vertex stage of mw_ocean_displace_mesh, sampled
 *                  the same way (resolution^2 vertices) at the handle's CURRENT phase.  UNITS: per second of delta_time: the phase
 *                  advances by omega * delta_time * mult, so the spectrum is weighted by omega * mult.  The handle keeps only its latest phase, so frame is -1
 *                  or the last frame of the latest steps call while no later call (a single frame, mw_ocean_advance_phase,
 *                  mw_ocean_set_phase, ...) has moved the phase; any other frame is MW_EINVAL.  After mw_ocean_advance_phase /
 *                  mw_ocean_set_phase the current phase is the new one, ahead of the latest textures.
 * mw_ocean_velocity: velocity_xyz [R*R*3], R = grid size (FFTMesh) or resolution (OceanRenderer), vertex layout of the outputs.
 * mw_ocean_query_velocity: the point located EXACTLY as mw_ocean_query_surface locates it (same arguments, same modes, same walk;
 *   residuals bit-identical), out [n][4] = vx, vy, vz, residual: the velocity of the water particle at the located rest point u*,
 *   the vertex velocities of u*'s triangle interpolated with the weights of the position.  A rest-mode query at a vertex returns
 *   that vertex's velocity bit for bit.  NaN where mw_ocean_query_surface gives NaN.
 * mw_ocean_query_velocity returns MW_ESTATE while the spectrum or phase has moved on since the latest frame (mw_ocean_set_spectrum,
 *   mw_ocean_reinit_spectrum, mw_ocean_set_phase, mw_ocean_advance_phase without a frame after them): the located surface and the
 *   velocity would belong to different instants.  mw_ocean_velocity answers for the current spectrum and phase.
 * Errors as mw_ocean_query_surface: MW_ESTATE before the first frame; MW_EINVAL for a batched handle, a bad mode or frame, iterations
 * outside [0,64], a NULL array, n out of range (mw_tiles_* handles: use the tile's own handle, single oceans only).
 * No velocity call changes the handle's state (timer, phase, latest frame, frame textures); the weighted spectrum is built on first use
 * into buffers of the handle, rebuilt after mw_ocean_set_spectrum / mw_ocean_reinit_spectrum, and freed by mw_ocean_destroy.       */
mw_status mw_ocean_velocity(mw_ocean* o, int32_t frame, float* velocity_xyz); /* host, synchronous */
mw_status mw_ocean_velocity_device(mw_ocean* o, int32_t frame, void* d_velocity_xyz); /* device array, async on the handle's stream */
/* xz [n][2], out [n][4]: host arrays, synchronous */
mw_status mw_ocean_query_velocity(mw_ocean* o, int32_t frame, int32_t mode, const float* xz, int64_t n, int32_t iterations,
                                  float* out);
/* device arrays (d_xz 8-byte, d_out 16-byte aligned), asynchronous on the handle's stream */
mw_status mw_ocean_query_velocity_device(mw_ocean* o, int32_t frame, int32_t mode, const void* d_xz, int64_t n,
                                         int32_t iterations, void* d_out);

/* ---- hull forces: buoyancy and drag on floating bodies -----------------------------------------------------------
 * The force and torque the water exerts on nbodies instances of one hull, from the displaced surface mw_ocean_query_surface reads
 * and, with drag on, the velocity mw_ocean_query_velocity reads.  No rigid-body integration: the caller applies the result
 *   (or mw_ocean_step_bodies integrates it on the device).
 * Hull: one triangle mesh in body space, hull_xyz [nverts][3], triangles [ntris][3] (int32), shared by all bodies.  (b - a) x (c - a)
 *   points OUT of the hull (the numeric convention of Unity's RecalculateNormals: a Unity mesh passes as it is).  The mesh need not
 *   be closed, but the buoyancy is exactly Archimedes (rho g V_submerged through the centre of buoyancy, on flat water) only for a
 *   closed mesh.
 * Bodies: bodies [nbodies][16] floats (64 B per body; 16-byte aligned in the device form) = px py pz _ | qx qy qz qw | vx vy vz _ |
 *   wx wy wz _: the reference point p (normally the centre of mass), the rotation q (normalised here), the linear velocity v and the
 *   angular velocity w, all in the object space of the ocean's vertex outputs (the space of query xz).  Instance vertex x = p + R(q) h,
 *   its velocity v + w x (x - p).
 * Water at a vertex: eta = the world-mode query_surface height at (x.x, x.z), located exactly as that query locates it (same frame and
 *   iterations, same walk), u = the water velocity at the same located point times velocity_scale (1 / t_division for FFTMesh gives
 *   per-second units, 1 for OceanRenderer), depth d = eta - x.y.  The water velocity is the surface particle's at every depth (an
 *   approximation: no attenuation of the orbital velocity with depth).
 * Hydrostatics per triangle: the triangle clipped at d = 0 by linear interpolation along its edges (0, 1 or 2 submerged sub-triangles;
 *   corners at d = 0 count as dry), per sub-triangle with corners x_i, depths d_i >= 0, D = sum d_i, S = (x1 - x0) x (x2 - x0) / 2,
 *   r_i = x_i - p:  F = -rho g (D / 3) S,  tau = -(rho g / 12) (sum d_i r_i + D sum r_i) x S  -- the exact integrals of the linear
 *   pressure rho g d over the sub-triangle.
 * Drag per submerged sub-triangle, at its centroid c, area A, n = S / A: v_rel = v + w x (c - p) - u(c) (u at cut points interpolated
 *   along the edge like d), F_lin = -linear_drag A v_rel, F_quad = -quadratic_drag A max(0, v_rel . n)^2 n (faces advancing into the
 *   water only), tau = (c - p) x (F_lin + F_quad).
 * coeffs [MW_HULL_NCOEFFS] (a host array in both forms) = density, gravity, linear_drag, quadratic_drag, velocity_scale.
 * out [nbodies][8] = Fx Fy Fz wetted_area tx ty tz residual: total force, the summed area A of the submerged sub-triangles, torque
 *   about p, and the largest world-mode residual over the body's vertices (NaN-propagating: it flags folds and hulls off the
 *   footprint).  A body with a non-finite vertex, or a vertex whose query has no answer, gets a row of NaN; a body entirely above the
 *   water gets exact zeros and its residual.  Every row is bitwise reproducible and independent of nbodies: body k alone gives the
 *   bits body k gives in any batch.
 * Frame and state: with linear_drag = quadratic_drag = 0 no velocity is computed and the rules are mw_ocean_query_surface's (frame -1,
 *   or k of the latest OceanRenderer steps call); with drag on they are mw_ocean_query_velocity's, MW_ESTATE included once the spectrum
 *   or phase moved past the latest frame.  The call changes nothing of the handle's state; its buffers (a vertex slab and per-chunk
 *   partial sums) grow on demand and are freed by mw_ocean_destroy.
 * MW_EINVAL for a batched handle, a NULL array with nbodies > 0 (coeffs always), nverts < 3 or ntris < 1, nbodies < 0,
 *   nbodies * nverts or nbodies * ntris above 2^31 - 256, a negative or non-finite coefficient, a bad frame or iterations (as the
 *   queries).  The host form also checks the triangle indices; in the device form an index outside [0, nverts) makes every row NaN
 *   (the kernel checks each index and reads nothing out of range).  nbodies == 0 does nothing.                                  */
#define MW_HULL_NCOEFFS 5
/* host arrays, synchronous */
mw_status mw_ocean_hull_forces(mw_ocean* o, int32_t frame, const float* hull_xyz, int32_t nverts, const int32_t* triangles,
                               int32_t ntris, const float* bodies, int32_t nbodies, const float* coeffs, int32_t iterations,
                               float* out);
/* device arrays (d_hull_xyz, d_triangles 4-byte, d_bodies, d_out 16-byte aligned), asynchronous on the handle's stream; coeffs host */
mw_status mw_ocean_hull_forces_device(mw_ocean* o, int32_t frame, const void* d_hull_xyz, int32_t nverts, const void* d_triangles,
                                      int32_t ntris, const void* d_bodies, int32_t nbodies, const float* coeffs,
                                      int32_t iterations, void* d_out);

/* ---- floating bodies: step many rigid hulls on the ocean in one call ---------------------------------------------
 * mw_ocean_step_bodies advances nbodies instances of one hull by dt under the forces mw_ocean_hull_forces computes, in `substeps`
 * substeps, on the device: the state crosses the API once per call, not once per substep.
 * Inputs: frame, hull_xyz / triangles, iterations and coeffs [MW_HULL_NCOEFFS] (density, gravity, linear_drag, quadratic_drag,
 *   velocity_scale) mean exactly what they mean in mw_ocean_hull_forces; gravity also accelerates the bodies (along -y).  The hull must
 *   be expressed about the centre of mass p (mw_hull_mass_properties gives the centroid to subtract).  bodies [nbodies][16] (p _ q v _
 *   w _, as in mw_ocean_hull_forces) is updated in place; floats 3, 11 and 15 of a body pass through unchanged.  mass [nbodies]
 *   [MW_BODY_NMASS] = m Ixx Iyy Izz Ixy Ixz Iyz 0: the mass and the inertia tensor's entries about p in body axes (Ixy = -int xy dm).
 *   out [nbodies][8] is optional (NULL allowed): the hull-forces row of the LAST substep, evaluated at the state at its start.
 * Integrator: semi-implicit Euler with h = dt / substeps (computed once in f32).  Each substep, in this order:
 *   1. the row (F, A, tau) at the current state, exactly as mw_ocean_hull_forces computes it;
 *   2. v <- v + h (F / m + (0, -g, 0)),  g = coeffs[1];
 *   3. w <- w + h I_w^-1 (tau - w x (I_w w)),  I_w = R I_b R^T, I_w^-1 = R I_b^-1 R^T, R the rotation of q;
 *   4. p <- p + h v;
 *   5. q <- normalize(q + (h / 2) (w, 0) (x) q).
 * Frozen surface: every substep reads the same frame's surface and, with drag on, the same velocity field, computed once per call;
 *   the caller advances the ocean between calls.  The frame and state rules are mw_ocean_hull_forces', MW_ESTATE included.  The call
 *   changes nothing of the handle's state; its buffers grow on demand and are freed by mw_ocean_destroy.
 * Failures: a substep whose row is NaN (a vertex off the footprint, a non-finite pose, a bad device index) leaves the body with the bits
 *   it had at the start of that substep for the rest of the call, and its out row is NaN.  A mass row is invalid when m <= 0 or not
 *   finite, or when I_b is not positive definite in f32 (leading minors): the host form returns MW_EINVAL naming the body, the device
 *   form gives that body a NaN row and leaves its state unchanged.
 * MW_EINVAL for substeps outside [1, 64], a negative or non-finite dt, a NULL mass with nbodies > 0, the argument rules of
 *   mw_ocean_hull_forces (out excepted) and misalignment (device form: d_hull_xyz and d_triangles 4-byte, d_bodies, d_mass and d_out
 *   16-byte aligned).  nbodies == 0 does nothing.
 * Reproducibility: a body's result depends only on its own inputs: it has the same bits alone as in a batch of any size.
 * mw_hull_mass_properties (host arrays, no device needed): out[10] = mass, cx cy cz (the centroid, hull space), Ixx Iyy Izz Ixy Ixz
 *   Iyz (the inertia tensor's entries about the centroid, hull axes; Ixy = -int xy dm) of the closed hull (outward winding) of uniform
 *   density; sums in f64.  MW_EINVAL for a NULL array, nverts < 3 or ntris < 1, a bad index, a density not finite and > 0, or a
 *   volume that is not positive (an open or inward-wound mesh).                                                                    */
#define MW_BODY_NMASS 8   /* mass row: m Ixx Iyy Izz Ixy Ixz Iyz 0 -- about the centre of mass p, body axes */
mw_status mw_hull_mass_properties(const float* hull_xyz, int32_t nverts, const int32_t* triangles, int32_t ntris, float density,
                                  float* out);
/* host arrays, synchronous */
mw_status mw_ocean_step_bodies(mw_ocean* o, int32_t frame, const float* hull_xyz, int32_t nverts, const int32_t* triangles,
                               int32_t ntris, float* bodies, const float* mass, int32_t nbodies, const float* coeffs, float dt,
                               int32_t substeps, int32_t iterations, float* out);
/* device arrays, asynchronous on the handle's stream; coeffs host */
mw_status mw_ocean_step_bodies_device(mw_ocean* o, int32_t frame, const void* d_hull_xyz, int32_t nverts, const void* d_triangles,
                                      int32_t ntris, void* d_bodies, const void* d_mass, int32_t nbodies, const float* coeffs,
                                      float dt, int32_t substeps, int32_t iterations, void* d_out);

/* ---- moorings: step floating bodies tethered to anchors by lines ---------------------------------------------------
 * mw_ocean_step_moored is mw_ocean_step_bodies with up to MW_MOORING_MAX_LINES lines per body, each from a point of the body to a fixed
 *   anchor.  A line's force depends on the pose and velocity of the body at every substep, so it is computed inside the substep loop, on
 *   the device: the state still crosses the API once per call.
 * lines [nbodies][lines_per_body][MW_MOORING_NLINE], lines_per_body = K in [1, MW_MOORING_MAX_LINES].  One slot is three float4:
 *     hx hy hz L0 | ax ay az k | c _ _ _
 *   h: the attachment point in body space, about p, like the hull.  L0 >= 0: the unstretched length.  a: the anchor in the object space
 *   of the bodies (world).  k >= 0: the stiffness.  c >= 0: the damping along the line.  The last three floats are padding and are not
 *   read.  A slot with k == 0 and c == 0 is empty and is skipped.
 * Per substep, at the state at its start (the state the water row is evaluated at), for every non-empty slot in slot order:
 *   1. x = p + R(q) h, R the rotation the hull vertices use;   2. va = v + w x (x - p);   3. r = a - x, l = |r|;
 *   4. l <= L0: the line is slack and contributes nothing (l == 0 included);
 *   5. e = r / l, T = max(0, k (l - L0) - c (va . e)): a line pulls and never pushes;   6. F = T e, tau = (x - p) x F.
 *   (x - p is evaluated as R(q) h, before p is added.)  The body's mooring wrench M is the sum of the taut slots' (F, tau) in slot order,
 *   starting from the first taut slot's own value.  With at least one slot taut, steps 2 and 3 of the integrator see F[k] + M[k] and
 *   tau[k] + M[4+k], one float32 add each, exactly as mw_ocean_step_fleet adds a wrench.  With no slot taut the water row is used as
 *   it is, no addition: a call whose lines all stay slack or empty leaves the bits of the unmoored call on a periodic handle and with
 *   draught on (on the one footprint without draught mw_ocean_step_bodies integrates with contraction and this call strictly: equal to
 *   rounding there).  out still reports the water row alone.  All of it is strict float32.
 * tension [nbodies][lines_per_body] is optional (NULL allowed): each slot's T at the start of the last substep, 0 for a slack or
 *   empty slot.
 * Stability: the integrator is the semi-implicit Euler of mw_ocean_step_bodies.  It needs h sqrt(k_total / m) < 2, h = dt / substeps,
 *   for the stiffest direction (k_total the summed stiffness of the lines along it).  The library does not check this.
 * Invalid slots: a slot is invalid when one of its nine used floats is not finite or L0, k or c is negative.  It is treated like an
 *   invalid mass row: the host form returns MW_EINVAL naming body and slot, the device form gives that body a NaN out row and NaN
 *   tensions and leaves its state unchanged.  The NaN-row rule of mw_ocean_step_bodies is unchanged, and a body whose last substep had
 *   a NaN row reports NaN tensions beside its NaN out row: a pose that is not known says nothing about its lines.
 * Everything else -- frame, state, argument, alignment and size rules, "changes nothing of the handle's state", the periodic switch and
 *   the draught switch -- is mw_ocean_step_bodies'.  In addition MW_EINVAL for lines_per_body outside [1, MW_MOORING_MAX_LINES] or a
 *   NULL lines with nbodies > 0; device form: d_lines 16-byte, d_tension 4-byte aligned.
 * Plans: on a periodic handle without draught the call follows mw_ocean_step_bodies' plan rule (one launch for hulls of fewer than 4
 *   chunks, per substep above); on a non-periodic handle and with draught on it always steps per substep.  The bits are the same.
 * Lines on a mixed fleet, and body-to-body lines (tow lines): mw_ocean_step_rigged, below the fleets.                               */
#define MW_MOORING_MAX_LINES 8
#define MW_MOORING_NLINE 12   /* slot: hx hy hz L0 | ax ay az k | c _ _ _ */
/* host arrays, synchronous */
mw_status mw_ocean_step_moored(mw_ocean* o, int32_t frame, const float* hull_xyz, int32_t nverts, const int32_t* triangles,
                               int32_t ntris, float* bodies, const float* mass, const float* lines, int32_t lines_per_body,
                               int32_t nbodies, const float* coeffs, float dt, int32_t substeps, int32_t iterations, float* out,
                               float* tension);
/* device arrays, asynchronous on the handle's stream; coeffs host */
mw_status mw_ocean_step_moored_device(mw_ocean* o, int32_t frame, const void* d_hull_xyz, int32_t nverts, const void* d_triangles,
                                      int32_t ntris, void* d_bodies, const void* d_mass, const void* d_lines, int32_t lines_per_body,
                                      int32_t nbodies, const float* coeffs, float dt, int32_t substeps, int32_t iterations,
                                      void* d_out, void* d_tension);

/* ---- mixed fleets: forces and stepping for many hull shapes in one call ---------------------------------------------
 * mw_ocean_fleet_forces and mw_ocean_step_fleet are mw_ocean_hull_forces and mw_ocean_step_bodies for a whole scene: up to
 *   MW_FLEET_MAX_HULLS hull shapes, each with its own coefficients and its own bodies, in one call.  The velocity field (drag on) is
 *   computed once per call and every substep takes one set of launches, whatever the number of shapes.
 * Geometry: hull_xyz [total_verts][3] and triangles [total_tris][3] hold every hull's geometry, concatenated.  Triangle indices are
 *   local to their hull, in [0, nverts_h).  Two hulls may share a vertex or a triangle range.
 * hulls [nhulls][MW_FLEET_NHULL] = vert_first, nverts, tri_first, ntris, nbodies: a HOST array in both forms, like coeffs.  nhulls in
 *   [1, MW_FLEET_MAX_HULLS]; each range inside its array; nverts >= 3, ntris >= 1; nbodies >= 0 (a hull without bodies is allowed); the
 *   hulls' nbodies add up to total_bodies.
 * Per-body arrays: the bodies lie hull after hull in table order in bodies [total_bodies][16], mass [total_bodies][MW_BODY_NMASS],
 *   wrench [total_bodies][8] and out [total_bodies][8]; a row means what it means in the single-hull entry points (out of step_fleet is
 *   optional, NULL allowed).
 * coeffs [nhulls][MW_HULL_NCOEFFS]: a HOST array, one row of density, gravity, linear_drag, quadratic_drag, velocity_scale per hull.
 *   Drag is on for the call when any hull's row has drag: the frame and state rules are then mw_ocean_query_velocity's, MW_ESTATE
 *   included, otherwise mw_ocean_query_surface's.  A hull whose own row has no drag reads no velocity.
 * The defining property: the out row of a body, and after step_fleet its state, has the bits mw_ocean_hull_forces or
 *   mw_ocean_step_bodies gives on that body's hull alone with that hull's coeffs row and the same frame, iterations, dt and substeps --
 *   in the host and device forms, on periodic and non-periodic handles, in both semantics.  A row therefore does not depend on which
 *   other hulls and bodies are in the fleet, or on their order.
 * wrench (step_fleet; optional, NULL = none): per body Fx Fy Fz _ tx ty tz _, an external force and a torque about p in world axes,
 *   constant over the call's substeps.  It is added to the water row before steps 2 and 3 of the integrator (F[k] + wrench[k] and
 *   tau[k] + wrench[4+k], one float32 add each); out still reports the water row alone.  With wrench == NULL there is no addition and
 *   the bits are mw_ocean_step_bodies'; an all-zero wrench promises nothing (-0 + 0 changes a sign).  A non-finite wrench row is
 *   treated like an invalid mass row: the host form returns MW_EINVAL naming the body, the device form gives that body a NaN out row
 *   and leaves its state unchanged.
 * Failures stay local: the NaN-row rule and the invalid-mass rule of mw_ocean_step_bodies apply per body.  In the device forms a
 *   triangle index outside [0, nverts_h) makes NaN rows for the bodies of that hull only; the host forms check every hull's indices
 *   and return MW_EINVAL naming the hull.  A body off the one footprint of a non-periodic handle is NOT a NaN row: as in the
 *   single-hull calls the world-mode walk clamps to the mesh's edge, the row is that of the edge's water and its residual is the
 *   distance to it; the other bodies are not affected.  On a periodic handle the body is in another tile.
 * Plans: on a periodic handle mw_ocean_step_fleet follows mw_ocean_step_bodies' plan rule hull by hull (hulls of fewer than 4 chunks
 *   of 256 triangles and vertices in one launch for all substeps, the others per substep).  On a non-periodic handle it always
 *   steps per substep, whatever the library's plan switch says: the bits are the same, but for a fleet of one or two small hull
 *   shapes the call is slower than mw_ocean_step_bodies on each (DESIGN.md section 7i has the figures).
 * MW_EINVAL for a broken hull-table rule; total_bodies, sum nbodies_h * nverts_h or sum nbodies_h * ntris_h above 2^31 - 256; a NULL
 *   array with total_bodies > 0 (hulls and coeffs always); a negative or non-finite coefficient; a batched handle; and the substeps,
 *   dt, frame, iterations and alignment rules of the single-hull calls (d_wrench 16-byte aligned).  total_bodies == 0 does nothing.
 *   Caller arrays are untouched on failure; nothing of the handle's state changes.  The calls share the single-hull calls' buffers.
 * Mooring and tow lines on a fleet: mw_ocean_step_rigged, below.                                                                     */
#define MW_FLEET_MAX_HULLS 32
#define MW_FLEET_NHULL 5   /* hull row: vert_first, nverts, tri_first, ntris, nbodies */
/* host arrays, synchronous */
mw_status mw_ocean_fleet_forces(mw_ocean* o, int32_t frame, const float* hull_xyz, int32_t total_verts, const int32_t* triangles,
                                int32_t total_tris, const int32_t* hulls, int32_t nhulls, const float* bodies, int32_t total_bodies,
                                const float* coeffs, int32_t iterations, float* out);
/* device arrays, asynchronous on the handle's stream; hulls and coeffs host */
mw_status mw_ocean_fleet_forces_device(mw_ocean* o, int32_t frame, const void* d_hull_xyz, int32_t total_verts, const void* d_triangles,
                                       int32_t total_tris, const int32_t* hulls, int32_t nhulls, const void* d_bodies,
                                       int32_t total_bodies, const float* coeffs, int32_t iterations, void* d_out);
/* host arrays, synchronous */
mw_status mw_ocean_step_fleet(mw_ocean* o, int32_t frame, const float* hull_xyz, int32_t total_verts, const int32_t* triangles,
                              int32_t total_tris, const int32_t* hulls, int32_t nhulls, float* bodies, const float* mass,
                              const float* wrench, int32_t total_bodies, const float* coeffs, float dt, int32_t substeps,
                              int32_t iterations, float* out);
/* device arrays, asynchronous on the handle's stream; hulls and coeffs host */
mw_status mw_ocean_step_fleet_device(mw_ocean* o, int32_t frame, const void* d_hull_xyz, int32_t total_verts, const void* d_triangles,
                                     int32_t total_tris, const int32_t* hulls, int32_t nhulls, void* d_bodies, const void* d_mass,
                                     const void* d_wrench, int32_t total_bodies, const float* coeffs, float dt, int32_t substeps,
                                     int32_t iterations, void* d_out);

/* ---- rigged fleets: mooring lines and tow lines on a mixed fleet in one call --------------------------------------------
 * mw_ocean_step_rigged is mw_ocean_step_fleet plus lines, targets, lines_per_body and tension: every body of a mixed fleet carries up
 *   to MW_MOORING_MAX_LINES lines, each to a fixed anchor (mw_ocean_step_moored's line) or to a point of another body of the call (a tow
 *   line).  Everything not stated here is mw_ocean_step_fleet's rule.
 * lines [total_bodies][lines_per_body][MW_MOORING_NLINE], lines_per_body = K in [1, MW_MOORING_MAX_LINES]: mw_ocean_step_moored's slot,
 *   hx hy hz L0 | ax ay az k | c _ _ _, with its validity rule; a slot with k == 0 and c == 0 is empty and is skipped.
 * targets [total_bodies][lines_per_body], int32, optional (NULL: every slot is anchored).  MW_RIG_ANCHOR: a is a fixed point of the
 *   bodies' object space, exactly as in mw_ocean_step_moored.  j >= 0: a is an attachment point in the body space of body j, an index
 *   into the call's bodies array.  The target of an empty slot is not read.
 * tension [total_bodies][lines_per_body] is optional, with mw_ocean_step_moored's meaning.  wrench and out are optional as in
 *   mw_ocean_step_fleet; out still reports the water row alone.
 * Per substep every slot is evaluated at the state ALL bodies had at the start of that substep (a snapshot: no body sees another
 *   body's already-advanced state, so the result does not depend on the order of the bodies).  A tow slot of body i with target j:
 *   d_j = R(q_j) a, x_j = p_j + d_j, vb = v_j + w_j x d_j, the same expressions as the owner's d = R(q_i) h, x, va; then steps 3 to 6 of
 *   mw_ocean_step_moored with the anchor replaced by x_j (r = x_j - x) and the closing speed (va - vb) . e.  With MW_RIG_ANCHOR the slot
 *   is mw_ocean_step_moored's, bit for bit (vb is absent, not zero).
 * A line joining bodies i and j is written in both tables: body i holds (h_i; a = h_j; target j) and body j holds (h_j; a = h_i;
 *   target i), with the same L0, k and c.  Such mirrored slots give F_i == -F_j and T_i == T_j bitwise at every substep: r, va - vb and e
 *   of the two ends are exact negations, l and T equal bits.  The library does NOT check mirroring: a one-sided slot pulls only its
 *   owner, which suits a scripted tug whose own motion is prescribed.  Lines are Euclidean in the bodies' object space; on a periodic
 *   handle nothing wraps.
 * The body's line wrench M is the slot-order sum of its taut slots, as in mw_ocean_step_moored.  The integrator sees (F + W) + M: first
 *   the wrench add of mw_ocean_step_fleet, when wrench != NULL, then the M add, when a slot is taut; no add happens for an absent part.
 *   With targets NULL or all MW_RIG_ANCHOR and wrench NULL every body has mw_ocean_step_moored's bits on its hull alone; with no slot
 *   taut the call has mw_ocean_step_fleet's bits on a periodic handle (equal to rounding on the one footprint, where this call
 *   integrates strictly).  All of it is strict float32.
 * Failures stay local.  A body is invalid for the call when a non-empty slot's target lies outside [-1, total_bodies) or is the body's
 *   own index, or a slot is invalid.  It is treated like an invalid mass row: the host form returns MW_EINVAL naming body and slot, the
 *   device form gives that body a NaN out row and NaN tensions and leaves its state unchanged, and reads nothing out of range.  A
 *   non-empty tow slot whose target's state holds a non-finite float among p, q, v, w at the start of a substep makes that substep a
 *   NaN-row substep of the owner: the owner keeps its bits for the rest of the call, with a NaN out row and NaN tensions.  A neighbour
 *   that is held or invalid is simply read at its unchanged state: failures do not spread beyond the bodies tied to a non-finite one.
 * Plans: the call always steps per substep, on every surface and whatever the library's plan switch says: a tow slot reads another
 *   body's state at the start of the substep, which one workgroup per body cannot see without a grid-wide barrier.  The substeps read
 *   the state from one array and write it to another, the caller's bodies and a buffer of the handle in turn.
 * MW_EINVAL in addition to mw_ocean_step_fleet's: lines_per_body outside [1, MW_MOORING_MAX_LINES]; a NULL lines with total_bodies > 0;
 *   device form: d_lines 16-byte, d_targets and d_tension 4-byte aligned.  Draught on: MW_ESTATE, as every fleet entry point.          */
#define MW_RIG_ANCHOR (-1)
/* host arrays, synchronous */
mw_status mw_ocean_step_rigged(mw_ocean* o, int32_t frame, const float* hull_xyz, int32_t total_verts, const int32_t* triangles,
                               int32_t total_tris, const int32_t* hulls, int32_t nhulls, float* bodies, const float* mass,
                               const float* wrench, const float* lines, const int32_t* targets, int32_t lines_per_body,
                               int32_t total_bodies, const float* coeffs, float dt, int32_t substeps, int32_t iterations, float* out,
                               float* tension);
/* device arrays, asynchronous on the handle's stream; hulls and coeffs host */
mw_status mw_ocean_step_rigged_device(mw_ocean* o, int32_t frame, const void* d_hull_xyz, int32_t total_verts, const void* d_triangles,
                                      int32_t total_tris, const int32_t* hulls, int32_t nhulls, void* d_bodies, const void* d_mass,
                                      const void* d_wrench, const void* d_lines, const void* d_targets, int32_t lines_per_body,
                                      int32_t total_bodies, const float* coeffs, float dt, int32_t substeps, int32_t iterations,
                                      void* d_out, void* d_tension);

/* ---- raycasts: where does this ray hit the water? -----------------------------------------------------------------
 * The first hit of each of n rays on the surface mw_ocean_query_surface reads, under its frame rules: FFTMesh frame -1 (the latest
 *   frame); OceanRenderer -1 or frame k of the latest steps call.  Triangles: rest cell (i, j), i along x and j along z, holds the lower
 *   triangle A B C = (i,j) (i+1,j) (i,j+1) and the upper triangle (i+1,j+1) (i+1,j) (i,j+1); triangle id = 2 * (i * (R-1) + j) + upper,
 *   R the grid size (FFTMesh) or resolution (OceanRenderer), vertex (i, j) at i * R + j.
 * rays [n][8] = ox oy oz tmin | dx dy dz tmax: the ray o + t d, t in units of d (d need not be unit length); a hit counts when
 *   tmin <= t <= tmax, tmax = +inf allowed.  A segment p0 -> p1 is o = p0, d = p1 - p0, tmin = 0, tmax = 1.  A ray is invalid when o or
 *   d is not finite, d = 0, tmin < 0, tmin > tmax, or tmin or tmax is NaN.
 * Intersection: two-sided and watertight (Woop, Benthin and Wald 2013); every float32 operation is uncontracted and correctly rounded.
 *   Per ray: kz = the axis of largest |d| (lowest index on ties), kx = (kz+1)%3, ky = (kx+1)%3, kx and ky swapped when d[kz] < 0;
 *     Sx = d[kx]/d[kz], Sy = d[ky]/d[kz], Sz = 1/d[kz].
 *   Per vertex P: P' = P - o; Px = P'[kx] - Sx*P'[kz], Py = P'[ky] - Sy*P'[kz], Pz = Sz*P'[kz].
 *   Per triangle A B C: U = Cx*By - Cy*Bx, V = Ax*Cy - Ay*Cx, W = Bx*Ay - By*Ax, each recomputed in float64 from the same float32
 *     values and rounded to float32 when it is exactly 0.  A hit when U, V and W are all >= 0 or all <= 0 and det = (U+V)+W != 0;
 *     t = ((U*Az + V*Bz) + W*Cz) / det; the barycentric weights of A, B and C are U/det, V/det and W/det.
 *   Each edge value is Qx*Py - Qy*Px of the edge's directed corners P -> Q.  A shared edge enters its two triangles in the same or in
 *   opposite directions, so its two values are equal or exact negatives, and no ray slips between two triangles.
 * First hit: the smallest accepted t over all triangles, ties to the smallest triangle id: a pure function of (mesh, ray), independent
 *   of n, of the ray's place in the batch and of the acceleration structure.
 * out [n][8] = t px py pz nx ny nz white: p = o + t d; the vertex normals interpolated with the hit's weights, then normalised (the
 *   triangle's map is affine, so these are the rest-plane weights query_surface uses); white the whitecap channel, same weights.
 * hit [n][2] int32 (optional, NULL allowed) = triangle id, facing: +1 when d . n_g < 0 in float64, n_g the displaced triangle's
 *   geometric normal oriented as the rest triangle's +y (lower: (P(i,j+1) - P(i,j)) x (P(i+1,j) - P(i,j)); upper: (P(i+1,j) -
 *   P(i+1,j+1)) x (P(i,j+1) - P(i+1,j+1))): the ray met the water from above; -1 otherwise: from below.
 * A miss gives t = +inf, NaN in the other 7 floats and hit (-1, 0); an invalid ray NaN in all 8 and (-1, 0).  The status is MW_OK.
 * MW_ESTATE before the first frame; MW_EINVAL for a batched handle, a bad frame, a NULL rays or out array with n > 0, n < 0 or
 *   n > 2^32 - 256, and in the device form d_rays or d_out not 16-byte aligned or d_hit not 8-byte aligned.  n == 0 does nothing.
 * Every call builds a bounds hierarchy of the surface on the handle's stream, in a buffer of the handle that
 *   grows on demand and is freed by mw_ocean_destroy; the call changes nothing of the handle's state.                          */
/* host arrays, synchronous */
mw_status mw_ocean_raycast(mw_ocean* o, int32_t frame, const float* rays, int64_t n, float* out, int32_t* hit);
/* device arrays, asynchronous on the handle's stream */
mw_status mw_ocean_raycast_device(mw_ocean* o, int32_t frame, const void* d_rays, int64_t n, void* d_out, void* d_hit);

/* ---- tiled raycasts: first hit of rays on the periodic ocean surface ------------------------------------------------
 * mw_ocean_raycast on the tiled surface of "the periodic surface" above.  The entry point names its surface: it does not read the
 *   periodic switch, gives the same bits with the switch on or off and leaves the switch and all other handle state alone.  It needs a
 *   grid that repeats: mw_ocean_get_periodic reporting P > 0.
 * Surface: vertex (gi, gj) of the integer grid, g = k*N + a (floor division), is vertex (ai, aj) of the frame displaced by
 *   (ki*P, 0, kj*P): x + (float)k * P in float32, k = 0 leaving the bits alone.  Every integer cell exists, the seam cells a = N-1
 *   (between the frame's last grid line and the next tile's first) included, split along the same diagonal as mw_ocean_raycast's cells.
 *   Tile (kx, kz) owns the N x N cells whose lower grid lines are its own.  Tiled triangle id = 2 * (ai*N + aj) + upper, in [0, 2 N^2);
 *   for ai, aj < N-1 it is mw_ocean_raycast's id of the same triangle + 2*ai.
 * rays [n][8]: the layout and the validity rule of mw_ocean_raycast.  A ray is also invalid when its origin lies more than 2^20 tiles
 *   from the base tile on x or z.  An invalid ray gives NaN in all 8 floats and hit (-1, 0, 0, 0).
 * Reduction first: K0 = the tile of the origin, ox = ox' + K0x*P with ox' in the base tile [rest(0), rest(0) + P] (likewise z).  The ray
 *   is cast from o' = (ox', oy, oz') in the frame of K0, where relative tile k has its vertices displaced by k*P; p = o' + t d, and
 *   K0x*P and K0z*P are added to px and pz once, at the end.  Precision therefore falls off with the distance the ray travels, not with
 *   the distance from the world origin: moving the origin by whole tiles (where that is exact in float32) leaves t, id, facing, normal
 *   and whitecap bit-identical.  A vertex of a seam has one expression, in terms of its global grid line, so its sheared coordinates are
 *   the same bits from both sides and no ray slips through a seam.
 * Window: the ray sees the (2*reach + 1)^2 tiles within `reach` of K0 on each axis, reach in [0, MW_RC_MAX_REACH].  Geometry of tiles
 *   outside the window is NOT seen, not even where it overhangs into the window: a caller that needs the answer of the infinite tiling
 *   picks reach one larger than the distance (in tiles) it cares about.
 * First hit: the smallest accepted t over every triangle of every window tile; ties go to the smallest relative tile x, then tile z,
 *   then id.  A pure function of (frame, ray, reach): independent of n, of the ray's place in the batch and of the acceleration
 *   structure.  The intersection arithmetic is mw_ocean_raycast's: strict float32, the float64 fallback for a zero edge value.
 * out [n][8] = t px py pz nx ny nz white, as mw_ocean_raycast: normal and whitecap from the (wrapped) vertices with the hit's weights.
 * hit [n][4] int32 (optional, NULL allowed) = id, facing, tile_x, tile_z: the tiled id, the facing of mw_ocean_raycast, and the ABSOLUTE
 *   tile of the triangle's cell (K0 plus its relative tile).
 *   A miss: t = +inf, NaN in the other 7 floats, hit (-1, 0, 0, 0): nothing in the window was hit, and the ray ended (tmax) or left the
 *     height range of the surface before it left the columns the window's tiles reach.
 *   Out of reach: the same row with id -2: nothing in the window was hit, and the ray left those columns -- the window's own and as
 *     many beyond them as a tile's geometry overhangs its footprint, one for any sane ocean -- while still inside [tmin, tmax] and the
 *     surface's height range.  The infinite tiling may or may not be hit further on.
 * MW_EINVAL for a batched handle; MW_ESTATE for an OceanRenderer handle; MW_EINVAL for reach outside [0, MW_RC_MAX_REACH];
 *   MW_ENOTCOMMENSURATE where the grid does not repeat (the shipped N = 12 scene, an odd N); then MW_EINVAL for frame != -1, a NULL rays
 *   or out with n > 0, n < 0 or n > 2^32 - 256, and in the device form d_rays, d_out or d_hit not 16-byte aligned; MW_ESTATE before the
 *   first frame.  n == 0 does nothing.  Caller arrays are untouched on failure.
 * Every call builds the bounds hierarchy of one tile in the buffer mw_ocean_raycast uses; the call changes
 *   nothing of the handle's state.  A horizontal displacement of more than 7 periods is not followed.                          */
#define MW_RC_DEFAULT_REACH 16
#define MW_RC_MAX_REACH 1024
/* host arrays, synchronous */
mw_status mw_ocean_raycast_tiled(mw_ocean* o, int32_t frame, const float* rays, int64_t n, int32_t reach, float* out, int32_t* hit);
/* device arrays (d_rays, d_out, d_hit 16-byte aligned), asynchronous on the handle's stream */
mw_status mw_ocean_raycast_tiled_device(mw_ocean* o, int32_t frame, const void* d_rays, int64_t n, int32_t reach, void* d_out,
                                        void* d_hit);

/* ---- the water column: water velocity and rest depth below the surface -------------------------------------------------
 * FFTMesh handles, every grid path.  A deep-water component of wave number k decays as e^{-k d} at rest depth d, and every output of a
 *   frame is linear in the spectrum: the water resting at depth d is one more frame, on the spectrum (A h0, A h0c) with A = e^{-k d},
 *   and its velocity one more velocity field, on (i w A h0, -i w A h0c).  In this Lagrangian first-order model the pressure on a
 *   material surface is rho g times its rest depth (exact for one trochoidal wave, first order for the sum), so the rest depth of the
 *   particle at a world point is the pressure there, under a crest or a trough alike.
 * A column is L layers, 2 <= L <= MW_COLUMN_MAX_LAYERS, at rest depths d_0 = 0 < d_1 < ... < d_{L-1}, all finite.  Layer 0 is not
 *   computed: it is the latest frame's mesh and mw_ocean_velocity's field, so the column agrees with the surface services by
 *   construction.  Layer l >= 1 of the latest frame (its t, its choppiness) is two [N*N][3] arrays: the frame's vertices on the
 *   attenuated spectrum, whose y holds the layer's height h_l above its own rest level (the layer's height is h_l - d_l), and its
 *   velocity in the units of mw_ocean_velocity.  Between layers every quantity is interpolated linearly, (1 - s) a + s b in strict
 *   float32; e^{-k d} is convex, so put the layers closer where the motion is large (geometric depths), and put the deepest layer where
 *   the motion the caller cares about has died out: below it the deepest layer's velocity is returned unchanged.
 * Memory: per layer below the surface two spectra (16 B per bin each; with their prep tables on the FFT path, 36 B per bin each) plus
 *   24 B per grid point, and once per column 16 B per grid point; allocated by the first column call after mw_ocean_set_column, freed by
 *   mw_ocean_set_column(o, NULL, 0) and mw_ocean_destroy.  The weighted spectra are rebuilt after mw_ocean_set_spectrum,
 *   mw_ocean_reinit_spectrum or mw_ocean_set_column, the layer arrays by the first column call after each frame.
 * mw_ocean_set_column: depths is a host array; nlayers == 0 (depths may be NULL) releases the column.  mw_ocean_get_column: either
 *   argument may be NULL; depths receives nlayers floats.
 * mw_ocean_column_layers: builds the layers if they are stale and returns the handle-owned device pointers of one layer, on the
 *   handle's stream, valid until the next frame, the next column or spectrum change, or destroy.  Layer 0 returns the surface mesh's
 *   vertex array and the handle's surface-velocity array.  Either output may be NULL.
 * mw_ocean_query_column: xyz_ [n][4] (the fourth float is ignored), out [n][12] =
 *     ux uy uz rest_depth | px py pz lambda | x0 z0 eta residual
 *   MW_QUERY_WORLD: (x, y, z) is a position in the water.  The layers are scanned from the top: in layer l, (x, z) is located exactly as
 *     mw_ocean_query_surface locates it on that layer's vertices (the caller's iterations, the same rules), which gives the layer's
 *     height y_l there, its velocity, the located rest point and a residual.  The scan stops at the first l with y > y_{l+1}; then
 *     y_{l+1} < y <= y_l and s = (y_l - y) / (y_l - y_{l+1}).  u, p (the reconstructed position) and the rest point (x0, z0) are blended
 *     between the two layers, rest_depth = (1 - s) d_l + s d_{l+1}, lambda = l + s, eta = y_0 (the surface height over the point),
 *     residual = the largest residual of the layers visited.  Layers below l + 1 are not located.  A point exactly on layer l
 *     (y == y_l, for instance py of mw_ocean_query_surface fed back) is that layer's sample: s = 0, lambda = l, rest_depth = d_l, and
 *     layer l + 1 is not located, so on the surface the residual is the surface's own.
 *       In the air (y > y_0): u = 0, rest_depth = y_0 - y (negative), lambda = 0; p, x0, z0, eta and residual are layer 0's.
 *       At or below the deepest layer (y <= y_{L-1}): the deepest layer's u, p, x0, z0; rest_depth = d_{L-1} + (y_{L-1} - y), the
 *         hydrostatic continuation; lambda = L - 1.
 *       A non-finite coordinate, or a layer whose locate has no answer, gives a row of NaN.
 *   MW_QUERY_REST: (x0, d, z0) is a particle's label: its rest-plane position and rest depth.  One rest-mode locate (the cell and the
 *     weights are the same in every layer); l is the last layer with d_l <= d, capped at L - 2, s = (d - d_l) / (d_{l+1} - d_l); p and u
 *     are blended between the two layers (p.y from h - d per layer), rest_depth = d, lambda = l + s, eta is layer 0's height at the
 *     label, residual = 0, and (x0, z0) come back as located.  d < 0, d > d_{L-1}, a label off the footprint or a non-finite input
 *     gives a row of NaN.  A label at a vertex's rest position with d = d_l returns that layer's vertex (y - d_l) and velocity bit for bit.
 *   A periodic handle (mw_ocean_set_periodic; the switch is read per call) reads every layer as the tiling: the point is reduced to the
 *     base tile, every layer gets the same tile indices, and the tile offset is added to px, pz, x0, z0 last.
 *   Arithmetic: strict float32 throughout, on every handle.  On a periodic handle eta and residual have the bits of
 *     mw_ocean_query_surface and, where lambda == 0, u the bits of mw_ocean_query_velocity; on a non-periodic handle they agree to
 *     rounding only, because those older kernels contract multiply-adds there.
 * MW_EINVAL: a NULL handle; an OceanRenderer or batched handle, which has no column (its mesh samples clamp-addressed textures);
 *   frame != -1; a bad mode; iterations outside [0, 64]; a NULL array with n > 0; n < 0 or n > 2^32 - 256; in the device form d_xyz_ or
 *   d_out not 16-byte aligned; nlayers outside {0} and [2, 16]; depths[0] != 0, or depths that are not strictly increasing or not
 *   finite; a layer out of range.
 * MW_ESTATE: no column set; no frame yet; the spectrum or phase moved past the latest frame (the rule of mw_ocean_query_velocity).
 * MW_ENOMEM: an allocation failed; a half-built column frees its buffers and the next call starts again.
 * n == 0 does nothing.  Caller arrays are untouched on failure.  No column call changes the timer, the phase, the frame, the periodic
 *   switch or anything another service reads.                                                                              */
#define MW_COLUMN_MAX_LAYERS 16
mw_status mw_ocean_set_column(mw_ocean* o, const float* depths, int32_t nlayers);
mw_status mw_ocean_get_column(mw_ocean* o, float* depths, int32_t* nlayers);
mw_status mw_ocean_column_layers(mw_ocean* o, int32_t frame, int32_t layer, void** d_positions, void** d_velocities);
/* host arrays, synchronous */
mw_status mw_ocean_query_column(mw_ocean* o, int32_t frame, int32_t mode, const float* xyz_, int64_t n, int32_t iterations, float* out);
/* device arrays (both 16-byte aligned), asynchronous on the handle's stream */
mw_status mw_ocean_query_column_device(mw_ocean* o, int32_t frame, int32_t mode, const void* d_xyz_, int64_t n, int32_t iterations,
                                       void* d_out);

/* ---- draught: hull forces and bodies read the water column below them ---------------------------------------------
 * Without draught every hull vertex gets the depth eta - y and the surface particle's velocity, however deep it lies: right for a barge,
 *   wrong for a keel, a spar buoy or a ship whose bottom sits a sizeable fraction of a wavelength down (the wave pressure under a hull
 *   of draught T is overstated by e^{kT}, the Smith effect, and the drag acts against water that does not move that fast down there).
 * mw_ocean_set_draught(o, 1) is a switch on the handle, like mw_ocean_set_periodic: read per call, default 0, and the entry points and
 *   array layouts of the hull family do not change.  With it on, mw_ocean_hull_forces, mw_ocean_step_bodies and their _device forms
 *   take every instance vertex as a world point of the column (the MW_QUERY_WORLD rules of mw_ocean_query_column, the caller's
 *   iterations): its depth is the point's rest_depth, so the pressure is rho g rest_depth, its water velocity (drag on) the column's u
 *   times velocity_scale, its residual the column's.  A vertex in the air carries eta - y and no velocity as before, so the waterline is
 *   still cut at depth 0; below the deepest layer the depth continues hydrostatically and the velocity is the deepest layer's.  A vertex
 *   the column has no answer for makes the body's row NaN.  The clip, the integrals, the order of the sum, the substep chain and every
 *   NaN rule are those of the calls without draught.  Periodic and draught combine: the layers are read as the tiling.
 *   Arithmetic: strict float32 throughout, on every handle (the column's).  On flat water the rows are Archimedes' as before.
 *   Stepping builds the layers once per call and runs every hull per substep (MW_BODIES_PLAN is not read).
 * With draught on the four calls take, after their own argument checks, the column's state rules whether drag is on or off:
 *   MW_ESTATE when no column is set (mw_ocean_set_column) or the spectrum or phase moved past the latest frame.
 * With draught on mw_ocean_fleet_forces, mw_ocean_step_fleet and their _device forms return MW_ESTATE before any other work: fleets do
 *   not read the column yet.  Queries, velocity, raycasts and the column query ignore the switch.
 * With draught off every call behaves, and launches, exactly as if the switch did not exist.
 * mw_ocean_set_draught: MW_EINVAL for a NULL handle, on outside {0, 1}, or a handle mw_ocean_set_column refuses (OceanRenderer,
 *   batched).  No column has to be set yet.  mw_ocean_get_draught: on may be NULL.                                              */
mw_status mw_ocean_set_draught(mw_ocean* o, int32_t on);                      /* 0 / 1; default 0 */
mw_status mw_ocean_get_draught(mw_ocean* o, int32_t* on);

/* ---- independent tiles on several devices (BASELINE configs[2]) ------------------------------------
 * Tiles are independent units in both semantics: tile k is the ocean of `params` with seed params->seed + k on its own
 * device, compute stream and output buffers; there is no data-path collective.  FFTMesh tiles advance up to max_steps
 * independent time-steps per mw_tiles_evaluate; OceanRenderer tiles up to max_steps CONSECUTIVE frames per
 * mw_tiles_generate_texture_steps (mw_ocean_generate_texture_steps_device per tile; max_steps <= 32 in both semantics).
 * The only exchange is the optional gather of finished outputs to one root device over RCCL (xGMI), issued on per-device SIDE streams behind an event recorded on
 * the compute streams -- once per batch, never per step (29.4 MB per 1024^2 tile ~ 190 us on one 153 GB/s link).
 *   single process : mw_tiles_create -- one RCCL rank per distinct device (ncclCommInitAll, rccl.h:236); tiles that share
 *                    a device share its rank.  devices == NULL places tile k on device k % mw_device_count().
 *   one process per GPU (the torch.distributed.run launch of bench.py): rank 0 calls mw_comm_unique_id, the launcher
 *                    broadcasts the 128 bytes, every rank calls mw_tiles_create_rank (ncclCommInitRank, rccl.h:220) and
 *                    owns exactly one tile; mw_tiles_gather is then collective over the ranks.
 * RCCL is loaded with dlopen on first use (no link-time dependency); MW_EDEVICE when it is absent.                     */
typedef struct mw_tiles mw_tiles;
#define MW_COMM_ID_BYTES 128
mw_status mw_comm_unique_id(void* id_out); /* MW_COMM_ID_BYTES bytes (ncclGetUniqueId) */
mw_status mw_tiles_create(const mw_params* params, int32_t ntiles, const int32_t* devices, int32_t max_steps, mw_tiles** out);
mw_status mw_tiles_create_rank(const mw_params* params, int32_t device, int32_t max_steps, const void* comm_id, int32_t rank,
                               int32_t nranks, mw_tiles** out);
void mw_tiles_destroy(mw_tiles* t);
int32_t mw_tiles_count(const mw_tiles* t);       /* tiles in the whole job (= nranks in the per-process form) */
int32_t mw_tiles_local_count(const mw_tiles* t); /* tiles this process owns */
mw_ocean* mw_tiles_ocean(mw_tiles* t, int32_t local_k); /* borrowed handle of a local tile (set_spectrum, set_choppiness, ...) */
/* nsteps <= max_steps time-steps t[0..nsteps) on every local tile (mw_ocean_evaluate_device per tile, asynchronous) */
mw_status mw_tiles_evaluate(mw_tiles* t, const float* times, int32_t nsteps, uint32_t flags);
/* device pointers of local tile k's outputs of the LATEST mw_tiles_evaluate: [max_steps][N*N*3], [max_steps][N*N*3],
 * [max_steps][N*N*(1|4)].  A tile that is gathered owns two such sets used alternately (the gather sends straight from the set
 * the latest evaluate wrote while the next evaluate fills the other one -- no snapshot copy): ask again after every evaluate
 * once mw_tiles_gather is in use.  Without gathers the pointers never change.                                              */
mw_status mw_tiles_outputs(mw_tiles* t, int32_t local_k, void** d_vertices, void** d_normals, void** d_white);
/* OceanRenderer tiles: one GenerateTexture() (S/OceanRenderer.cs:216) on every local tile, asynchronous; the result textures
 * of local tile k stay in its handle: height [M*M], disp_xz [M*M*2], normal_xyz [M*M*3], white [M*M].                  */
mw_status mw_tiles_generate_texture(mw_tiles* t, float delta_time);
mw_status mw_tiles_textures(mw_tiles* t, int32_t local_k, void** d_height, void** d_disp_xz, void** d_normal_xyz, void** d_white);
/* OceanRenderer tiles created with max_steps > 1: nframes <= max_steps consecutive frames on every local tile in one enqueue per tile
 * (delta_time[nframes]: HOST array), asynchronous.  mw_tiles_frames: the frames of local tile k, height [max_steps][M*M], disp_xz
 * [max_steps][M*M*2], normal_xyz [max_steps][M*M*3], white [max_steps][M*M] (stable pointers; MW_ESTATE when max_steps is 1);
 * mw_tiles_textures stays the latest frame.  mw_tiles_gather(step) then collects FRAME `step` of the latest call.               */
mw_status mw_tiles_generate_texture_steps(mw_tiles* t, const float* delta_time, int32_t nframes);
mw_status mw_tiles_frames(mw_tiles* t, int32_t local_k, void** d_height, void** d_disp_xz, void** d_normal_xyz, void** d_white);
/* Collect step `step` of EVERY tile (OceanRenderer: frame `step` of the latest call; 0 with max_steps 1) on the device of tile `root` (global tile
 * index): asynchronous, on the side streams.  mw_tiles_gathered: the root's buffer, per tile [N*N*3 | N*N*3 | N*N*w] floats
 * (OceanRenderer: [M*M | M*M*2 | M*M*3 | M*M]); NULL on processes that do not own root.  All multi-device entry points put
 * the caller's current HIP device back before they return.                                                           */
mw_status mw_tiles_gather(mw_tiles* t, int32_t step, int32_t root);
mw_status mw_tiles_gathered(mw_tiles* t, void** d_gathered, int64_t* floats_per_tile);
mw_status mw_tiles_synchronize(mw_tiles* t); /* compute and side streams of every local tile */

/* ---- pond: Gerstner vertex displacement  (W/MistralWaterLib.cginc:71-99,154-180) ---------------
 * pos_xyz/out_xyz [nverts*3] world positions; waves [nwaves*3] = {dir.x, dir.y, speed}; amplitude is
 * the already x0.01-scaled _Amplitude (:172).  out = pos + offsets (:176).  Host pointers, synchronous. */
mw_status mw_gerstner_displace(const float* pos_xyz, int64_t nverts, const float* waves, int32_t nwaves,
                               float amplitude, float frequency, float steepness, float t, float* out_xyz,
                               int32_t device);
/* device-pointer form, asynchronous on hip_stream (NULL = default stream) */
mw_status mw_gerstner_displace_device(const void* d_pos_xyz, int64_t nverts, const float* waves, int32_t nwaves,
                                      float amplitude, float frequency, float steepness, float t, void* d_out_xyz,
                                      void* hip_stream);

/* many time values of one lattice in ONE launch (the positions are read once, the time part of every wave's phase is
 * joined by angle addition): t[nsteps] is a HOST array, d_out_xyz is [nsteps][nverts*3].  nwaves must be 4 or 8 and
 * nsteps * nwaves <= 256 (mw_gerstner_max_steps); otherwise MW_EINVAL.  Asynchronous on hip_stream.               */
mw_status mw_gerstner_displace_steps_device(const void* d_pos_xyz, int64_t nverts, const float* waves, int32_t nwaves,
                                            float amplitude, float frequency, float steepness, const float* t,
                                            int32_t nsteps, void* d_out_xyz, void* hip_stream);
int32_t mw_gerstner_max_steps(int32_t nwaves); /* 0 when this wave count has no batched kernel */

/* ---- pond: the material's whole vertex-stage Displacement()  (W/MistralWaterLib.cginc:154-180) with every
 * displacement mode of the shader library.  Fields are the material properties of W/MistralWaterProperty.cginc /
 * W/MistralWaterLib.cginc:53-66 under their own names; `amplitude` is the raw _Amplitude (the x0.01 of :134/:172 is
 * applied inside, as the shader does).  Object space = world space.                                             */
#define MW_POND_WAVE 0               /* Wave(), :127-152: y only, finite-difference normal with _Smoothing        */
#define MW_POND_GERSTNER 1           /* Gerstner(), :71-99: 4 waves = _WDirectionAB.xy/.zw, _WDirectionCD.xy/.zw  */
#define MW_POND_GERSTNER_LEVEL_ONE 2 /* GerstnerLevelOne(), :101-125: 5 built-in waves                           */
typedef struct mw_pond_params {
    int32_t mode;
    float amplitude, frequency, speed, steepness, smoothing; /* _Amplitude _Frequency _Speed _Steepness _Smoothing */
    float wspeed[4];                                         /* _WSpeed                                           */
    float dir_ab[4], dir_cd[4];                              /* _WDirectionAB, _WDirectionCD                      */
} mw_pond_params;
/* out_xyz = displaced vertex, out_normal_xyz (may be NULL) = v.normal as the shader leaves it.  Host pointers,
 * synchronous; t = _Time.y.                                                                                      */
mw_status mw_pond_displace(const mw_pond_params* p, const float* pos_xyz, int64_t nverts, float t, float* out_xyz,
                           float* out_normal_xyz, int32_t device);
/* device-pointer form, asynchronous on hip_stream (NULL = default stream) */
mw_status mw_pond_displace_device(const mw_pond_params* p, const void* d_pos_xyz, int64_t nverts, float t,
                                  void* d_out_xyz, void* d_out_normal_xyz, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* MISTRAL_WATER_H */
