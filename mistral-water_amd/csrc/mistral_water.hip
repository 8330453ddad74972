// mistral_water.hip -- libmistral_water.so: gfx950 kernels + the C ABI of include/mistral_water.h.
//
// HIP-only product path: there is no CPU fallback anywhere in this file.  The CPU oracle lives in
// /oracle and is never linked here.
#include <hip/hip_runtime.h>

#include <dlfcn.h>  // tiles.inc binds RCCL at run time (dlopen / dlsym)

#include <algorithm>
#include <array>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <chrono>
#include <vector>

#include "../../include/mistral_water.h"
#include "../../include/mistral_water_hooks.h"
#include "mw_host.h"  // fail(), HIP_TRY, dmalloc, MW_FOR_SIZE
#include "fftmesh_kernels.h"
#include "ocean_renderer_device.h"
#include "direct_kernels.h"
#include "gerstner_kernels.h"
#include "pond_kernels.h"
#include "surface_query.h"
#include "velocity_kernels.h"
#include "hull_forces.h"
#include "rigid_bodies.h"
#include "fleet.h"
#include "surface_tiled.h"
#include "raycast.h"
#include "water_column.h"
#include "hull_draught.h"
static_assert(MW_COL_MAX_LAYERS == MW_COLUMN_MAX_LAYERS, "water_column.h and the ABI size the layer table alike");
static_assert(MW_SQ_REST == MW_QUERY_REST && MW_SQ_WORLD == MW_QUERY_WORLD, "surface_query.h and the ABI name the modes alike");

#ifndef MW_WAVES_P1
#define MW_WAVES_P1 6  // min waves per SIMD the register allocator must leave room for (measured best)
#endif
#ifndef MW_WAVES_P2
#define MW_WAVES_P2 6
#endif

using namespace mw;

#include "fftmesh_device.h"  // the FFTMesh kernels and FmState: here, where the kernels stand in the code object

// ------------------------------------------------------------------------------------------------
// handle
// ------------------------------------------------------------------------------------------------
// a grow-only device buffer of the handle: allocated at the largest size asked for so far, not per call (grow_reserve)
struct GrowBuf { void* p = nullptr; size_t cap = 0; };
// The water column of a handle (mw_ocean_set_column, water_column.h): the depths, and per layer below the surface the attenuated spectrum,
// its velocity-weighted twin (each with its k_prep tables on the FFT path) and the two vertex arrays of the latest frame.  Allocated on
// the first build, freed as a whole (col_release) when an allocation fails half-way, the column is replaced or the handle destroyed.
// ready: the weighted spectra belong to the handle's current spectrum; built: pos / vel belong to the latest frame -- both cleared by the
// frame-record functions below and set by column_spectra_built / column_layers_built.
struct ColLayer { FmSpectrum psp, vsp; float *pos = nullptr, *vel = nullptr; };
struct ColState {
    int L = 0;  // 0: no column
    float depth[MW_COL_MAX_LAYERS] = {};
    ColLayer layer[MW_COL_MAX_LAYERS];  // layer[0] stays empty: layer 0 is the surface mesh and vel.vert
    float *norm = nullptr, *white = nullptr;  // the normals / whitecap the frame kernels also write (unused)
    bool ready = false, built = false;
};
// frees every buffer, keeps the depths: the next build allocates again
static void col_release(ColState& c) {
    for (ColLayer& y : c.layer) {
        fm_spectrum_free(y.psp); fm_spectrum_free(y.vsp); hipFree(y.pos); hipFree(y.vel);
        y = ColLayer();
    }
    hipFree(c.norm); hipFree(c.white);
    c.norm = c.white = nullptr;
    c.ready = c.built = false;
}
struct mw_ocean {
    mw_params p;
    int N = 0;          // synthesis grid size
    int sem = 0;
    int device = 0;
    bool use_fft = false;
    hipStream_t stream = nullptr;
    hipStream_t own_stream = nullptr;
    float timer = 0.f;
    FmState fm;  // FFTMesh state: spectrum, tables, exchange buffers and the host-API frame (fftmesh_device.h)
    int or_steps_tail = -1;  // OceanRenderer: the last frame of the latest steps call while the phase is still that frame's, else -1
    bool frame_behind = false;  // the spectrum or the phase changed after the latest frame was made (mw_ocean_query_velocity refuses)
    bool periodic = false;      // mw_ocean_set_periodic: the surface services read the tiling of the frame (not part of the frame record)
    bool draught = false;       // mw_ocean_set_draught: hull forces and bodies read the water column (hull_draught.h; not part of the frame record)
    VelState vel;            // mw_ocean_velocity: the weighted spectrum and the velocity buffers (velocity_kernels.h)
    ColState col;            // mw_ocean_set_column: the layers below the surface (water_column.h)
    // five separate buffers: the host forms keep their staged inputs in scratch while hull, bodies and rc_tree are in use
    GrowBuf hull;     // mw_ocean_hull_forces: vertex slab + chunk partials (hull_forces.h)
    GrowBuf bodies;   // mw_ocean_step_bodies, per-substep plan: the rows of a substep [nbodies][8]
    GrowBuf rig;      // mw_ocean_step_rigged: the second state array of the substeps' pair [total_bodies][16] (rigging.h)
    GrowBuf rc_tree;  // mw_ocean_raycast: the bounds hierarchy of the queried surface (raycast.h), rebuilt every call
    GrowBuf scratch;  // device staging of the host-pointer entry points (Stage)
    float* q_mesh = nullptr;  // OceanRenderer surface queries: the vertex stage of the queried frame, [res^2][3 + 3 + 1], allocated on first use
    DirectState direct;
    // OceanRenderer state
    OrState orr;
};

static bool is_pow2(int n) { return n > 0 && (n & (n - 1)) == 0; }

// b holds at least `bytes` afterwards; growing waits for the work on the handle's stream that may still read the old buffer
static mw_status grow_reserve(mw_ocean* o, GrowBuf& b, size_t bytes, const char* what) {
    if (b.cap >= bytes) return MW_OK;
    if (b.p) {
        HIP_TRY(hipStreamSynchronize(o->stream));
        HIP_TRY(hipFree(b.p));
        b.p = nullptr;
        b.cap = 0;
    }
    if (hipMalloc(&b.p, bytes) != hipSuccess) return fail(MW_ENOMEM, std::string("hipMalloc of ") + what + " failed");
    b.cap = bytes;
    return MW_OK;
}
static mw_status scratch_reserve(mw_ocean* o, size_t bytes) { return grow_reserve(o, o->scratch, bytes, "the host-API staging buffer"); }
static size_t align256(size_t b) { return (b + 255) & ~(size_t)255; }

// Device staging of one host-pointer call in the handle's scratch buffer.  The call declares its arrays in order (in / out / inout:
// copied to the device before the launches, back after them, or both); each region starts on a 256-byte boundary.  begin() reserves
// the sum, sets every declared device pointer and issues the copies in; finish() issues the copies out and waits for the stream.  All
// copies run on the handle's stream in declaration order.  An array the caller left out (NULL) gets no region and a NULL device pointer.
// A stage holds as many regions as its declaration has arrays: Stage<N> st(o) followed by at most N in / out / inout, or, for a call
// record that lists its arrays (Arr; the surface services), Stage st(o, record.arrays()), whose N is the list's own length.
namespace {  // internal linkage: at file scope Stage::begin / finish would join the library's exported symbols
// One array of a call record, declared once: the record's pointer to it (the caller's going in, the staged copy's after begin()), its
// size, which way the host form copies it, and the alignment the device form asks of it (a power of two).
enum Dir { IN, OUT, INOUT };
struct Arr { void** slot; size_t bytes; Dir dir; uintptr_t align; };
template <size_t N>
struct Stage {
    struct Region { void** dev; const void* in; void* out; size_t bytes, off; };
    mw_ocean* o;
    Region r[N];
    size_t n = 0;
    size_t total = 0;
    explicit Stage(mw_ocean* o_) : o(o_) {}
    Stage(mw_ocean* o_, const std::array<Arr, N>& arrays) : o(o_) {
        for (const Arr& a : arrays) {
            void* host = *a.slot;
            add(a.slot, a.dir != OUT ? host : nullptr, a.dir != IN ? host : nullptr, a.bytes);
        }
    }
    void add(void** dev, const void* in, void* out, size_t bytes) {
        *dev = nullptr;
        if (!in && !out) return;
        if (n == N) std::abort();  // only a Stage<N> st(o) given more than its N arrays gets here: stop before writing past r[]
        const size_t off = align256(total);
        r[n++] = Region{dev, in, out, bytes, off};
        total = off + bytes;
    }
    void in(void** dev, const void* host, size_t bytes) { add(dev, host, nullptr, bytes); }
    void out(void** dev, void* host, size_t bytes) { add(dev, nullptr, host, bytes); }
    void inout(void** dev, void* host, size_t bytes) { add(dev, host, host, bytes); }
    mw_status begin() {
        mw_status s = scratch_reserve(o, total);
        if (s != MW_OK) return s;
        for (size_t k = 0; k < n; k++) *r[k].dev = static_cast<char*>(o->scratch.p) + r[k].off;
        for (size_t k = 0; k < n; k++)
            if (r[k].in) HIP_TRY(hipMemcpyAsync(*r[k].dev, r[k].in, r[k].bytes, hipMemcpyHostToDevice, o->stream));
        return MW_OK;
    }
    mw_status finish() {
        for (size_t k = 0; k < n; k++)
            if (r[k].out) HIP_TRY(hipMemcpyAsync(r[k].out, *r[k].dev, r[k].bytes, hipMemcpyDeviceToHost, o->stream));
        HIP_TRY(hipStreamSynchronize(o->stream));
        return MW_OK;
    }
};
}  // namespace

// ---- the frame record ----------------------------------------------------------------------------
// What the surface services may read -- s_have, s_wstride, s_t, s_chop, or_steps_tail, frame_behind, vel.ready, orr.frames_last,
// orr.fr_have -- is written by the functions below and nowhere else: every entry point that makes a frame, moves the phase or changes
// the spectrum calls the one that states what it did.
// velocity_spectrum_built below is the seventh writer: the only place vel.ready turns true (or_velocity sets its own for OceanRenderer).
// The water column hangs on the same record: a new or overwritten frame makes its layer arrays stale (col.built), a new spectrum its weighted
// spectra too (col.ready); column_spectra_built and column_layers_built are the only places the two turn true.
// an FFTMesh frame evaluated at time t now stands in s_vert / s_norm / s_white, its whitecap at stride wstride (4: RGBA colours, 1: scalar)
static void frame_fftmesh_made(mw_ocean* o, float t, int wstride) {
    o->fm.s_have = true; o->fm.s_wstride = wstride; o->fm.s_t = t; o->fm.s_chop = o->p.choppiness; o->frame_behind = false;
    o->col.built = false;
}
// the launches that follow overwrite s_vert / s_norm / s_white: they hold no frame until frame_fftmesh_made says so (profiling hook)
static void frame_fftmesh_overwritten(mw_ocean* o) { o->fm.s_have = false; o->col.built = false; }
// an OceanRenderer lone frame is being made: the latest frame is the phase's, and no frame of a steps call is
static void frame_or_lone(mw_ocean* o) { o->or_steps_tail = -1; o->frame_behind = false; }
// an OceanRenderer steps call made n frames and kept[k] says whether kind k (height, displacement, normal, whitecap) stayed in the
// handle; tail: the frame of that call the phase now belongs to (n - 1), or -1 when the caller cannot vouch for it
static void frame_or_steps(mw_ocean* o, int n, const bool kept[4], int tail) {
    for (int k = 0; k < 4; k++) o->orr.fr_have[k] = kept[k];
    o->orr.frames_last = n; o->or_steps_tail = tail; o->frame_behind = false;
}
// the OceanRenderer phase moved without a frame: no frame is the phase's any more
static void frame_phase_moved(mw_ocean* o) { o->or_steps_tail = -1; o->frame_behind = true; }
// the spectrum changed: the velocity spectrum derived from it is stale and the latest frame is not this spectrum's;
// phase_restarts: the OceanRenderer phase went back to 0 with it, so no frame of a steps call is the phase's either
static void frame_spectrum_changed(mw_ocean* o, bool phase_restarts) {
    o->vel.ready = false; o->frame_behind = true;
    o->col.ready = false; o->col.built = false;
    if (phase_restarts) o->or_steps_tail = -1;
}
// the velocity spectrum was rebuilt from the current spectrum (velocity_run; or_velocity does the same for OceanRenderer)
static void velocity_spectrum_built(mw_ocean* o) { o->vel.ready = true; }
// the column's weighted spectra were rebuilt from the current spectrum and depths; its layer arrays were built from the latest frame's
// time and choppiness (column_build)
static void column_spectra_built(mw_ocean* o) { o->col.ready = true; }
static void column_layers_built(mw_ocean* o) { o->col.built = true; }

// The four arrays that hold OceanRenderer frame k: the latest frame (k = -1), frame k of the latest steps call otherwise -- the handle's
// latest-frame textures too when that call made one frame (it ran the lone-frame plan), else slot k of the frame buffers.  A kind the
// steps call sent to caller buffers is NULL; complete: all four are here.
struct OrFrame { float* height; cf* disp; float *normal, *white; bool complete; };
static OrFrame or_frame(const OrState& r, int k) {
    if (k < 0) return OrFrame{r.out.height, r.out.disp, r.out.normal, r.out.white, true};
    const OrTex t = r.frames_last == 1 ? r.out : r.fr.at((size_t)k * r.M * r.M);
    const bool* have = r.fr_have;
    OrFrame f;
    f.height = have[0] ? t.height : nullptr;
    f.disp = have[1] ? t.disp : nullptr;
    f.normal = have[2] ? t.normal : nullptr;
    f.white = have[3] ? t.white : nullptr;
    f.complete = have[0] && have[1] && have[2] && have[3];
    return f;
}
// up to four device pointers through the optional out-arguments of an accessor entry point
static void store_ptrs(void** const (&out)[4], void* const (&p)[4]) { for (int k = 0; k < 4; k++) if (out[k]) *out[k] = p[k]; }

// concatenated twiddle table [TS1 | TS2 | TS3 | TF] in the layout of TwGeom<N,P>
namespace mw {
int plan_points_host(int N) { return N >= 2048 ? 16 : MW_PT; }
std::vector<cf> build_twiddle_table(int N, int P, int sgn) { return build_twiddle_table_host(N, P, sgn); }
}  // namespace mw

// The period of the handle's surface, or 0 where it does not repeat.  An FFTMesh frame tiles where the grid is commensurate and N is even
// (an odd N is anti-periodic); an OceanRenderer mesh samples clamp-addressed textures and never does.
static float grid_period(const mw_ocean* o) {
    if (o->sem != MW_SEM_FFTMESH || o->N % 2 != 0 || !(o->p.unit_width * (float)o->N == o->p.length)) return 0.f;
    return (float)o->N * o->p.unit_width;
}

static OceanConsts consts_of(const mw_ocean* o) { return OceanConsts{o->N, o->p.length, o->p.gravity, o->p.unit_width, o->p.choppiness}; }

// the prep tables of the handle's spectrum at the handle's length (FFT path; the direct-sum path has none)
static mw_status run_prep(mw_ocean* o) { return o->use_fft ? fm_prep(o->fm.sp, o->N, o->p.length, o->p.gravity, o->fm.Wpre, o->stream) : MW_OK; }

// FETCH_SIZE calibration streams (MI355X_MICROARCH.md "HBM": calibrate the counter on a known byte count in your own
// access width): every lane reads `width` bytes, lanes contiguous, `bytes` in total; one float per block is written.
// (mw_debug_stream_read, debug_hooks.inc; a template stands outside extern "C")
template <typename V>
__global__ void k_dbg_stream(const V* __restrict__ src, size_t n, float* sink) {
    float acc = 0.f;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        V v = src[i];
        acc += reinterpret_cast<const float*>(&v)[0];
    }
    if (acc == 123.456f) sink[blockIdx.x] = acc;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

int32_t mw_abi_version(void) { return MW_ABI_VERSION; }

// Identity of this build, fixed AT BUILD TIME: -DMW_BUILD_HASH = SHA-256 (first 16 hex digits) over the kernel sources, the two
// headers of the boundary and the compile flags, computed by the build recipe (mistral_water/_native.py::source_hash, the one
// place that knows them; tools/build_variant.sh calls the same function) + the tag the build gave it (-DMW_BUILD_TAG, "default"
// for the in-tree .so).  It names the code that is loaded, whatever happens to the file on disk afterwards.
#ifndef MW_BUILD_TAG
#define MW_BUILD_TAG "default"
#endif
// -DMW_LAB: a build for measurements (a knob overridden on the command line, cycle stamps, the plan switches taken from the environment).
// Its id says so, and bench.py and the tests refuse it unless told otherwise: a number or a green test always names a product build.
#ifdef MW_LAB
#define MW_BUILD_KIND "lab:"
#else
#define MW_BUILD_KIND ""
#endif
#ifndef MW_BUILD_HASH
#warning "MW_BUILD_HASH is not defined: build through mistral_water/_native.py::build_native or tools/build_variant.sh (mw_build_id() will say unhashed-build)"
#define MW_BUILD_HASH "unhashed-build"
#endif
const char* mw_build_id(void) { return MW_BUILD_HASH " " MW_BUILD_KIND MW_BUILD_TAG; }
const char* mw_last_error(void) { return g_err.c_str(); }

int32_t mw_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

void mw_params_default(mw_params* p, int32_t semantics) {
    if (!p) return;
    std::memset(p, 0, sizeof(*p));
    p->semantics = semantics;
    p->gravity = 9.81f;  // S/FFTMesh.cs:52
    p->seed = 1;
    if (semantics == MW_SEM_OCEANRENDERER) {  // S/OceanRenderer.cs:10-19
        p->mult = 2.f; p->unit_width = 1.f; p->resolution = 256; p->length = 256.f; p->choppiness = 1.5f;
        p->amplitude = 1.f; p->wind_x = 0.f; p->wind_y = 0.f; p->t_division = 1.f;
    } else {  // S/FFTMesh.cs:9-23
        p->choppiness = 1.f; p->t_division = 1.f; p->resolution = 50; p->unit_width = 1.f; p->length = 1.f;
        p->wind_x = 1.f; p->wind_y = 1.f; p->amplitude = 1.f; p->mult = 1.f;
    }
}

void mw_ocean_destroy(mw_ocean* o) {
    if (!o) return;
    hipSetDevice(o->device);
    if (hipStreamSynchronize(o->stream) != hipSuccess) (void)hipGetLastError();  // a dead caller stream has nothing pending
    hipFree(o->q_mesh);
    for (GrowBuf* b : {&o->scratch, &o->hull, &o->bodies, &o->rig, &o->rc_tree}) hipFree(b->p);
    vel_free(o->vel);
    col_release(o->col);
    direct_free(o->direct);
    fm_free(o->fm);
    or_free(o->orr);
    if (o->own_stream) hipStreamDestroy(o->own_stream);
    delete o;
}

static mw_status ocean_create_impl(const mw_params* params, int tiles, mw_ocean** out) {
    if (!params || !out) return fail(MW_EINVAL, "mw_ocean_create: NULL argument");
    *out = nullptr;
    if (tiles < 1 || tiles > 64) return fail(MW_EINVAL, "mw_ocean_create_batch: ntiles must be in [1,64]");
    if (tiles > 1 && params->semantics != MW_SEM_OCEANRENDERER)
        return fail(MW_EINVAL, "mw_ocean_create_batch: OceanRenderer semantics only (FFTMesh batches in time, mw_ocean_evaluate_device)");
    if (params->semantics != MW_SEM_FFTMESH && params->semantics != MW_SEM_OCEANRENDERER)
        return fail(MW_EINVAL, "mw_ocean_create: unknown semantics");
    if (params->resolution < 2) return fail(MW_EINVAL, "mw_ocean_create: resolution must be >= 2");
    if (!(params->length > 0.f) || !(params->gravity > 0.f))
        return fail(MW_EINVAL, "mw_ocean_create: length and gravity must be positive");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(MW_EDEVICE, "mw_ocean_create: no HIP device visible (this library has no CPU fallback)");
    if (params->device < 0 || params->device >= ndev) return fail(MW_EINVAL, "mw_ocean_create: bad device ordinal");
    HIP_TRY(hipSetDevice(params->device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, params->device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(MW_EDEVICE, std::string("mw_ocean_create: device is ") + prop.gcnArchName +
                                    ", this library carries gfx950 (MI355X) code only");

    mw_ocean* o = new (std::nothrow) mw_ocean();
    if (!o) return fail(MW_ENOMEM, "mw_ocean_create: out of host memory");
    o->p = *params;
    o->sem = params->semantics;
    o->device = params->device;
    mw_status s = MW_OK;
    hipError_t he = hipStreamCreateWithFlags(&o->own_stream, hipStreamNonBlocking);
    if (he != hipSuccess) { delete o; return fail(MW_EDEVICE, "hipStreamCreate failed"); }
    o->stream = o->own_stream;
    if (sw(SW_P1_TGROUP) >= 0) o->fm.p1_tgroup = sw(SW_P1_TGROUP);

    if (o->sem == MW_SEM_FFTMESH) {
        const int N = params->resolution;
        o->N = N;
        // FFT path precondition: power of two and unit_width == length / N exactly.
        o->use_fft = is_pow2(N) && N >= 64 && (params->unit_width * (float)N == params->length);
        if (N > 4096) s = fail(MW_EINVAL, "FFTMesh: resolution > 4096 unsupported");
        else if (o->use_fft || (s = direct_create(o->direct, N, params->unit_width, params->length, params->gravity, o->stream)) == MW_OK)
            s = fm_create(o->fm, *params, N, o->use_fft, o->stream);
    } else {
        const int M = params->resolution * 8;  // S/OceanRenderer.cs:136
        o->N = M;
        if (!is_pow2(M)) s = fail(MW_ENOTPOW2, "OceanRenderer: 8*resolution must be a power of two");
        else if (M < 64 || M > 4096) s = fail(MW_EINVAL, "OceanRenderer: texture size must be in [64,4096]");
        else s = or_create(o->orr, *params, M, o->stream, tiles);
    }
    if (s == MW_OK && (he = hipStreamSynchronize(o->stream)) != hipSuccess) s = fail(MW_EDEVICE, std::string("create sync: ") + hipGetErrorString(he));
    if (s != MW_OK) { mw_ocean_destroy(o); return s; }  // (the message the failing step left stands: nothing on the way out calls fail())
    *out = o;
    return MW_OK;
}

mw_status mw_ocean_create(const mw_params* params, mw_ocean** out) { return ocean_create_impl(params, 1, out); }
mw_status mw_ocean_create_batch(const mw_params* params, int32_t ntiles, mw_ocean** out) { return ocean_create_impl(params, ntiles, out); }
int32_t mw_ocean_batch_size(const mw_ocean* o) { return o ? (o->sem == MW_SEM_OCEANRENDERER ? o->orr.tiles : 1) : 0; }

// Drain the stream the handle is leaving.  A caller-owned stream may have been destroyed since (a garbage-collected
// torch.cuda.Stream): hipErrorInvalidHandle / ContextIsDestroyed then mean "nothing pending" -- the handle must still be able
// to leave the dead stream (and mw_ocean_destroy to finish).
static mw_status drain_stream(mw_ocean* o) {
    const hipError_t e = hipStreamSynchronize(o->stream);
    if (e == hipSuccess) return MW_OK;
    if (o->stream != o->own_stream &&
        (e == hipErrorInvalidHandle || e == hipErrorContextIsDestroyed || e == hipErrorInvalidResourceHandle)) {
        (void)hipGetLastError();  // clear the sticky error: it described the caller's stream, not this library's work
        return MW_OK;
    }
    return fail(MW_EDEVICE, std::string("hipStreamSynchronize(previous stream): ") + hipGetErrorString(e));
}
mw_status mw_ocean_set_stream(mw_ocean* o, void* hip_stream) {
    if (!o) return fail(MW_EINVAL, "NULL handle");
    HIP_TRY(hipSetDevice(o->device));
    mw_status s = drain_stream(o);
    if (s != MW_OK) return s;
    o->stream = reinterpret_cast<hipStream_t>(hip_stream);  // NULL = HIP's legacy default stream, like the pond entry points
    return MW_OK;
}
mw_status mw_ocean_use_own_stream(mw_ocean* o) {
    if (!o) return fail(MW_EINVAL, "NULL handle");
    HIP_TRY(hipSetDevice(o->device));
    mw_status s = drain_stream(o);
    if (s != MW_OK) return s;
    o->stream = o->own_stream;
    return MW_OK;
}
void* mw_ocean_get_stream(mw_ocean* o) { return o ? reinterpret_cast<void*>(o->stream) : nullptr; }
mw_status mw_ocean_synchronize(mw_ocean* o) {
    if (!o) return fail(MW_EINVAL, "NULL handle");
    HIP_TRY(hipSetDevice(o->device));
    HIP_TRY(hipStreamSynchronize(o->stream));
    return MW_OK;
}
mw_status mw_ocean_set_choppiness(mw_ocean* o, float c) {
    if (!o) return fail(MW_EINVAL, "NULL handle");
    o->p.choppiness = c;
    return MW_OK;
}

mw_status mw_ocean_set_periodic(mw_ocean* o, int32_t on) {
    const char* who = "mw_ocean_set_periodic";
    if (!o) return fail(MW_EINVAL, who, "NULL handle");
    if (on != 0 && on != 1) return fail(MW_EINVAL, who, "on must be 0 or 1");
    if (on) {
        if (o->sem == MW_SEM_OCEANRENDERER && o->orr.tiles != 1)
            return fail(MW_EINVAL, who, "a batched handle (mw_ocean_create_batch) has no single surface");
        if (o->sem != MW_SEM_FFTMESH)
            return fail(MW_ESTATE, who, "an OceanRenderer mesh does not tile (its edge vertices sample half a texel inside the texture): FFTMesh handles only");
        if (grid_period(o) == 0.f)
            return fail(MW_ENOTCOMMENSURATE, who, "the frame repeats only where unit_width * resolution == length and the resolution is even");
    }
    o->periodic = on != 0;
    return MW_OK;
}
mw_status mw_ocean_get_periodic(mw_ocean* o, int32_t* on, float* period) {
    if (!o) return fail(MW_EINVAL, "mw_ocean_get_periodic", "NULL handle");
    if (on) *on = o->periodic ? 1 : 0;
    if (period) *period = grid_period(o);
    return MW_OK;
}

int32_t mw_ocean_grid_size(const mw_ocean* o) { return o ? o->N : 0; }
int64_t mw_ocean_index_count(const mw_ocean* o) {
    if (!o) return 0;
    int64_t n = o->p.resolution;  // the MESH is resolution^2 in both modes (S/OceanRenderer.cs:132-135)
    return (n - 1) * (n - 1) * 6;
}
int32_t mw_ocean_max_batch(const mw_ocean* o) { return (o && o->sem == MW_SEM_FFTMESH && o->use_fft) ? MW_MAX_BATCH : 1; }
float mw_ocean_timer(const mw_ocean* o) { return o ? o->timer : 0.f; }
mw_status mw_ocean_reset_timer(mw_ocean* o) {
    if (!o) return fail(MW_EINVAL, "NULL handle");
    o->timer = 0.f;
    return MW_OK;
}

mw_status mw_ocean_set_spectrum(mw_ocean* o, const float* h0_xy, const float* h0conj_xy) {
    if (!o || !h0_xy || !h0conj_xy) return fail(MW_EINVAL, "mw_ocean_set_spectrum: NULL argument");
    HIP_TRY(hipSetDevice(o->device));
    frame_spectrum_changed(o, true);  // OceanRenderer: the phase restarts
    const int tiles = (o->sem == MW_SEM_OCEANRENDERER) ? o->orr.tiles : 1;
    const size_t bytes = sizeof(cf) * (size_t)o->N * o->N * tiles;
    if (o->sem == MW_SEM_OCEANRENDERER) {  // initialTexture.rg / .ba, texel (px,py) at py*M + px, tile-major
        void *a, *b;
        Stage<2> st(o);
        st.in(&a, h0_xy, bytes);
        st.in(&b, h0conj_xy, bytes);
        mw_status s = st.begin();
        if (s != MW_OK) return s;
        k_or_set_init<<<dim3((unsigned)(((size_t)o->N * o->N + 255) / 256), tiles), dim3(256), 0, o->stream>>>(
            o->N, static_cast<const cf*>(a), static_cast<const cf*>(b), o->orr.initT, o->orr.phaseT);
        k_or_prep<<<dim3((unsigned)(((size_t)o->N * o->N + 255) / 256), tiles), dim3(256), 0, o->stream>>>(o->N, o->orr.initT, o->orr.PQT);
        HIP_TRY(hipGetLastError());
        o->orr.phase_sym = true;  // a fresh spectrum restarts the phase at 0
        return st.finish();
    }
    HIP_TRY(hipMemcpyAsync(o->fm.sp.h0, h0_xy, bytes, hipMemcpyHostToDevice, o->stream));
    HIP_TRY(hipMemcpyAsync(o->fm.sp.h0c, h0conj_xy, bytes, hipMemcpyHostToDevice, o->stream));
    mw_status s = run_prep(o);
    if (s != MW_OK) return s;
    HIP_TRY(hipStreamSynchronize(o->stream));
    return MW_OK;
}
mw_status mw_ocean_get_spectrum(mw_ocean* o, float* h0_xy, float* h0conj_xy) {
    if (!o || !h0_xy || !h0conj_xy) return fail(MW_EINVAL, "mw_ocean_get_spectrum: NULL argument");
    HIP_TRY(hipSetDevice(o->device));
    const int tiles = (o->sem == MW_SEM_OCEANRENDERER) ? o->orr.tiles : 1;
    const size_t bytes = sizeof(cf) * (size_t)o->N * o->N * tiles;
    if (o->sem == MW_SEM_OCEANRENDERER) {
        void *a, *b;
        Stage<2> st(o);
        st.out(&a, h0_xy, bytes);
        st.out(&b, h0conj_xy, bytes);
        mw_status s = st.begin();
        if (s != MW_OK) return s;
        k_or_get_init<<<dim3((unsigned)(((size_t)o->N * o->N + 255) / 256), tiles), dim3(256), 0, o->stream>>>(o->N, o->orr.initT, static_cast<cf*>(a),
                                                                                                          static_cast<cf*>(b));
        HIP_TRY(hipGetLastError());
        return st.finish();
    }
    HIP_TRY(hipMemcpyAsync(h0_xy, o->fm.sp.h0, bytes, hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(hipMemcpyAsync(h0conj_xy, o->fm.sp.h0c, bytes, hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(hipStreamSynchronize(o->stream));
    return MW_OK;
}

mw_status mw_ocean_reinit_spectrum(mw_ocean* o, float length, float wind_x, float wind_y, float amplitude, uint64_t seed) {
    if (!o) return fail(MW_EINVAL, "NULL handle");
    if (!(length > 0.f)) return fail(MW_EINVAL, "mw_ocean_reinit_spectrum: length must be positive");
    HIP_TRY(hipSetDevice(o->device));
    frame_spectrum_changed(o, false);  // new spectrum and dispersion; the phase textures stay
    mw_status s;
    if (o->sem == MW_SEM_OCEANRENDERER) {  // S/OceanRenderer.cs:98-109: RenderInitial() again, phase textures untouched
        s = or_reinit(o->orr, length, wind_x, wind_y, amplitude, seed, o->stream);
    } else {
        if ((is_pow2(o->N) && o->N >= 64 && (o->p.unit_width * (float)o->N == length)) != o->use_fft)
            return fail(MW_ESTATE, "mw_ocean_reinit_spectrum: the new length moves the grid between the FFT and the direct-sum path; "
                                   "create a new handle");
        s = fm_reinit(o->fm, o->direct, o->p, o->N, o->use_fft, length, wind_x, wind_y, amplitude, seed, o->stream);
    }
    if (s != MW_OK) return s;
    o->p.length = length; o->p.wind_x = wind_x; o->p.wind_y = wind_y; o->p.amplitude = amplitude; o->p.seed = seed;
    if (grid_period(o) == 0.f) o->periodic = false;  // the new length no longer repeats with the grid: the tiling is gone
    HIP_TRY(hipStreamSynchronize(o->stream));
    return MW_OK;
}

// OceanRenderer: the length the normal pass uses (normalMat._Length, set once in SetParams, S/OceanRenderer.cs:163, and
// never again -- a later length change through mw_ocean_reinit_spectrum leaves it behind).  Part of the checkpoint:
// restoring (initialTexture, phase) into a fresh handle created with the CURRENT length must also restore this.
float mw_ocean_normal_length(const mw_ocean* o) {
    if (!o) return 0.f;
    return o->sem == MW_SEM_OCEANRENDERER ? o->orr.c.normal_length : o->p.length;
}
mw_status mw_ocean_set_normal_length(mw_ocean* o, float normal_length) {
    if (!o) return fail(MW_EINVAL, "NULL handle");
    if (o->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, "mw_ocean_set_normal_length: OceanRenderer semantics only");
    if (!(normal_length > 0.f)) return fail(MW_EINVAL, "mw_ocean_set_normal_length: must be positive");
    o->orr.c.normal_length = normal_length;
    return MW_OK;
}

static mw_status phase_copy(mw_ocean* o, float* host_out, const float* host_in, const char* who) {
    if (!o || (!host_out && !host_in)) return fail(MW_EINVAL, who, "NULL argument");
    if (o->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, who, "OceanRenderer semantics only (FFTMesh state is the timer)");
    HIP_TRY(hipSetDevice(o->device));
    const size_t MM = (size_t)o->N * o->N, bytes = MM * sizeof(float) * o->orr.tiles;
    mw_status s = scratch_reserve(o, bytes);
    if (s != MW_OK) return s;
    float* tmp = static_cast<float*>(o->scratch.p);
    const dim3 grid((unsigned)((MM + 255) / 256), o->orr.tiles), block(256);
    if (host_out) {  // device [px][py] -> host texel order py*M + px
        k_or_phase_transpose<<<grid, block, 0, o->stream>>>(o->N, o->orr.phaseT, tmp);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(host_out, tmp, bytes, hipMemcpyDeviceToHost, o->stream));
    } else {
        frame_phase_moved(o);
        HIP_TRY(hipMemcpyAsync(tmp, host_in, bytes, hipMemcpyHostToDevice, o->stream));
        k_or_phase_transpose<<<grid, block, 0, o->stream>>>(o->N, tmp, o->orr.phaseT);
        HIP_TRY(hipGetLastError());
        // The two-transform plan needs phase[p] == phase[m(p)], m the index mirror (csrc/ocean_renderer_kernels.h): true of every phase the library
        // produced (omega is mirror-symmetric bit for bit), checked for what a caller hands in -- anything else runs the three-transform plan
        bool sym = true;
        const int M = o->N;
        for (int t = 0; t < o->orr.tiles && sym; t++) {
            const float* ph = host_in + (size_t)t * MM;
            for (int py = 0; py < M && sym; py++) {
                const float* row = ph + (size_t)py * M;
                const float* mrow = ph + (size_t)((M - py) % M) * M;
                for (int px = 0; px < M; px++)
                    if (row[px] != mrow[(M - px) % M]) { sym = false; break; }
            }
        }
        o->orr.phase_sym = sym;
    }
    HIP_TRY(hipStreamSynchronize(o->stream));
    return MW_OK;
}
mw_status mw_ocean_get_phase(mw_ocean* o, float* phase) { return phase_copy(o, phase, nullptr, "mw_ocean_get_phase"); }
mw_status mw_ocean_set_phase(mw_ocean* o, const float* phase) { return phase_copy(o, nullptr, phase, "mw_ocean_set_phase"); }
mw_status mw_ocean_set_timer(mw_ocean* o, float timer) {
    if (!o) return fail(MW_EINVAL, "NULL handle");
    o->timer = timer;
    return MW_OK;
}

mw_status mw_ocean_rest_mesh(mw_ocean* o, float* vertices_xyz, float* normals_xyz, float* uvs_xy, int32_t* indices) {
    if (!o) return fail(MW_EINVAL, "NULL handle");
    HIP_TRY(hipSetDevice(o->device));
    const int N = o->p.resolution;  // mesh resolution (not the 8x texture size in OceanRenderer mode)
    const size_t NN = (size_t)N * N, nidx = (size_t)(N - 1) * (N - 1) * 6;
    void *dv, *dn, *du, *di;
    Stage<4> st(o);
    st.out(&dv, vertices_xyz, NN * 3 * sizeof(float));
    st.out(&dn, normals_xyz, NN * 3 * sizeof(float));
    st.out(&du, uvs_xy, NN * 2 * sizeof(float));
    st.out(&di, indices, nidx * sizeof(int32_t));
    mw_status s = st.begin();
    if (s != MW_OK) return s;
    hipLaunchKernelGGL(k_rest_mesh, dim3((unsigned)((NN + 255) / 256)), dim3(256), 0, o->stream, N, o->p.unit_width, static_cast<float*>(dv),
                       static_cast<float*>(dn), static_cast<float*>(du), static_cast<int32_t*>(di));
    HIP_TRY(hipGetLastError());
    return st.finish();
}

mw_status mw_ocean_evaluate_device(mw_ocean* o, const float* t, int32_t nsteps, void* d_vertices, void* d_normals,
                                   void* d_white, uint32_t flags) {
    if (!o || !t || !d_vertices || !d_normals || !d_white) return fail(MW_EINVAL, "mw_ocean_evaluate_device: NULL argument");
    if (o->sem != MW_SEM_FFTMESH) return fail(MW_ESTATE, "mw_ocean_evaluate_device: FFTMesh semantics only");
    if (nsteps < 1 || nsteps > mw_ocean_max_batch(o)) return fail(MW_EINVAL, "mw_ocean_evaluate_device: nsteps out of range");
    HIP_TRY(hipSetDevice(o->device));
    const int white_stride = (flags & MW_OUT_COLOR_RGBA) ? 4 : 1;
    if (!o->use_fft)
        return direct_evaluate(o->direct, consts_of(o), o->fm.sp.h0, o->fm.sp.h0c, t[0], (float*)d_vertices, (float*)d_normals, (float*)d_white,
                               white_stride, o->stream);
    return fm_evaluate(o->fm, o->fm.sp, consts_of(o), t, nsteps, (float*)d_vertices, (float*)d_normals, (float*)d_white, white_stride, o->stream);
}

mw_status mw_ocean_evaluate(mw_ocean* o, float t, float* vertices_xyz, float* normals_xyz, float* colors_rgba) {
    if (!o) return fail(MW_EINVAL, "NULL handle");
    if (o->sem != MW_SEM_FFTMESH) return fail(MW_ESTATE, "mw_ocean_evaluate: FFTMesh semantics only");
    mw_status s = mw_ocean_evaluate_device(o, &t, 1, o->fm.s_vert, o->fm.s_norm, o->fm.s_white, MW_OUT_COLOR_RGBA);
    if (s != MW_OK) return s;
    frame_fftmesh_made(o, t, 4);
    return fm_frame_to_host(o->fm, (size_t)o->N * o->N, vertices_xyz, normals_xyz, colors_rgba, nullptr, nullptr, o->stream);
}

mw_status mw_ocean_update(mw_ocean* o, float delta_time, float* vertices_xyz, float* normals_xyz, float* colors_rgba) {
    if (!o) return fail(MW_EINVAL, "NULL handle");
    o->timer += delta_time / o->p.t_division;  // S/FFTMesh.cs:70
    return mw_ocean_evaluate(o, o->timer, vertices_xyz, normals_xyz, colors_rgba);
}

// ---- OceanRenderer frames: planar / RGBA x one frame / steps x device / host --------------------------------------------------
// What the four device forms do once their arguments stand: n frames through or_frames, and the frame record.  A lone call's latest frame
// is the phase's; a steps call (n == 1 included: the lone-frame plan, its textures the handle's own) records what it kept.
static mw_status make_frames(mw_ocean* o, const float* delta_time, int n, bool steps, bool rgba, void* const (&d)[4]) {
    HIP_TRY(hipSetDevice(o->device));
    if (!steps) frame_or_lone(o);
    mw_status s = or_frames(o->orr, o->p.choppiness, delta_time, n, rgba, d, o->stream);
    if (s != MW_OK || !steps) return s;
    const bool kept[4] = {rgba || !d[0], rgba || !d[1], rgba || !d[2], rgba || !d[3]};  // what the caller did not take stays in the handle
    frame_or_steps(o, n, kept, n - 1);
    return MW_OK;
}
mw_status mw_ocean_generate_texture_device(mw_ocean* o, float delta_time, void* d_height, void* d_disp_xz,
                                           void* d_normal_xyz, void* d_white) {
    if (!o) return fail(MW_EINVAL, "NULL handle");
    if (o->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, "mw_ocean_generate_texture: OceanRenderer semantics only");
    return make_frames(o, &delta_time, 1, false, false, {d_height, d_disp_xz, d_normal_xyz, d_white});
}
mw_status mw_ocean_generate_texture_rgba_device(mw_ocean* o, float delta_time, void* d_height_rgba, void* d_disp_rgba,
                                                void* d_normal_rgba, void* d_white_rgba) {
    if (!o) return fail(MW_EINVAL, "NULL handle");
    if (o->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, "mw_ocean_generate_texture_rgba: OceanRenderer semantics only");
    return make_frames(o, &delta_time, 1, false, true, {d_height_rgba, d_disp_rgba, d_normal_rgba, d_white_rgba});
}
mw_status mw_ocean_generate_texture_steps_device(mw_ocean* o, const float* delta_time, int32_t nframes, void* d_height,
                                                 void* d_disp_xz, void* d_normal_xyz, void* d_white) {
    if (!o || !delta_time) return fail(MW_EINVAL, "mw_ocean_generate_texture_steps: NULL argument");
    if (o->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, "mw_ocean_generate_texture_steps: OceanRenderer semantics only");
    if (nframes < 1 || nframes > mw_ocean_max_frames(o))
        return fail(o->orr.tiles != 1 ? MW_ESTATE : MW_EINVAL, o->orr.tiles != 1 ? "mw_ocean_generate_texture_steps: a batched handle (mw_ocean_create_batch) advances one frame per call"
                                                                                 : "mw_ocean_generate_texture_steps: nframes out of range (mw_ocean_max_frames)");
    return make_frames(o, delta_time, nframes, true, false, {d_height, d_disp_xz, d_normal_xyz, d_white});
}
mw_status mw_ocean_generate_texture_steps_rgba_device(mw_ocean* o, const float* delta_time, int32_t nframes, void* d_height_rgba,
                                                      void* d_disp_rgba, void* d_normal_rgba, void* d_white_rgba) {
    if (!o || !delta_time) return fail(MW_EINVAL, "mw_ocean_generate_texture_steps_rgba: NULL argument");
    if (o->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, "mw_ocean_generate_texture_steps_rgba: OceanRenderer semantics only");
    if (nframes < 1 || nframes > mw_ocean_max_frames(o))
        return fail(o->orr.tiles != 1 ? MW_ESTATE : MW_EINVAL, "mw_ocean_generate_texture_steps_rgba: nframes out of range, or a batched handle");
    return make_frames(o, delta_time, nframes, true, true, {d_height_rgba, d_disp_rgba, d_normal_rgba, d_white_rgba});
}
// The host forms, once their arguments stand, around the device form of the same name.  Planar textures stay in the handle (the latest
// frame, or the frame buffers of a steps call) and leave from there over PCIe; the RGBA targets are staged.  host: [n][...] arrays.
static mw_status frames_to_host(mw_ocean* o, const float* delta_time, int n, bool steps, bool rgba, float* const (&host)[4]) {
    HIP_TRY(hipSetDevice(o->device));
    const size_t texels = (size_t)o->N * o->N * (size_t)(steps ? n : o->orr.tiles);
    void* dev[4] = {nullptr, nullptr, nullptr, nullptr};
    Stage<4> st(o);
    if (rgba) {
        for (int k = 0; k < 4; k++) st.out(&dev[k], host[k], texels * 4 * sizeof(float));
        mw_status s = st.begin();
        if (s != MW_OK) return s;
    }
    mw_status s = steps ? (rgba ? mw_ocean_generate_texture_steps_rgba_device(o, delta_time, n, dev[0], dev[1], dev[2], dev[3])
                                : mw_ocean_generate_texture_steps_device(o, delta_time, n, nullptr, nullptr, nullptr, nullptr))
                        : (rgba ? mw_ocean_generate_texture_rgba_device(o, delta_time[0], dev[0], dev[1], dev[2], dev[3])
                                : mw_ocean_generate_texture_device(o, delta_time[0], nullptr, nullptr, nullptr, nullptr));
    if (s != MW_OK) return s;
    if (rgba) return st.finish();
    const OrFrame f = or_frame(o->orr, steps ? 0 : -1);
    const void* const src[4] = {f.height, f.disp, f.normal, f.white};
    const size_t per[4] = {1, 2, 3, 1};
    for (int k = 0; k < 4; k++)
        if (host[k]) HIP_TRY(hipMemcpyAsync(host[k], src[k], texels * per[k] * sizeof(float), hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(hipStreamSynchronize(o->stream));
    return MW_OK;
}
mw_status mw_ocean_generate_texture(mw_ocean* o, float delta_time, float* height, float* disp_xz, float* normal_xyz,
                                    float* white) {
    if (!o) return fail(MW_EINVAL, "NULL handle");
    if (o->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, "mw_ocean_generate_texture: OceanRenderer semantics only");
    return frames_to_host(o, &delta_time, 1, false, false, {height, disp_xz, normal_xyz, white});
}
mw_status mw_ocean_generate_texture_rgba(mw_ocean* o, float delta_time, float* height_rgba, float* disp_rgba,
                                         float* normal_rgba, float* white_rgba) {
    if (!o) return fail(MW_EINVAL, "NULL handle");
    if (o->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, "mw_ocean_generate_texture_rgba: OceanRenderer semantics only");
    return frames_to_host(o, &delta_time, 1, false, true, {height_rgba, disp_rgba, normal_rgba, white_rgba});
}
static mw_status steps_to_host(mw_ocean* o, const float* delta_time, int32_t nframes, bool rgba, float* const (&host)[4], const char* who) {
    if (!o || !delta_time) return fail(MW_EINVAL, who, "NULL argument");
    if (o->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, who, "OceanRenderer semantics only");
    return frames_to_host(o, delta_time, nframes, true, rgba, host);
}
mw_status mw_ocean_generate_texture_steps(mw_ocean* o, const float* delta_time, int32_t nframes, float* height, float* disp_xz, float* normal_xyz,
                                          float* white) {
    return steps_to_host(o, delta_time, nframes, false, {height, disp_xz, normal_xyz, white}, "mw_ocean_generate_texture_steps");
}
mw_status mw_ocean_generate_texture_steps_rgba(mw_ocean* o, const float* delta_time, int32_t nframes, float* height_rgba, float* disp_rgba,
                                               float* normal_rgba, float* white_rgba) {
    return steps_to_host(o, delta_time, nframes, true, {height_rgba, disp_rgba, normal_rgba, white_rgba}, "mw_ocean_generate_texture_steps_rgba");
}
mw_status mw_ocean_advance_phase(mw_ocean* o, const float* delta_time, int32_t nframes) {
    if (!o || (!delta_time && nframes > 0)) return fail(MW_EINVAL, "mw_ocean_advance_phase: NULL argument");
    if (o->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, "mw_ocean_advance_phase: OceanRenderer semantics only (FFTMesh time is mw_ocean_set_timer)");
    if (nframes < 0) return fail(MW_EINVAL, "mw_ocean_advance_phase: nframes < 0");
    if (nframes == 0) return MW_OK;
    HIP_TRY(hipSetDevice(o->device));
    frame_phase_moved(o);
    return or_advance_phase(o->orr, delta_time, nframes, o->stream);
}
int32_t mw_ocean_max_frames(const mw_ocean* o) { return (o && o->sem == MW_SEM_OCEANRENDERER && o->orr.tiles == 1) ? MW_OR_MAX_FRAMES : 0; }
mw_status mw_ocean_frame_textures(mw_ocean* o, int32_t frame, void** d_height, void** d_disp_xz, void** d_normal_xyz, void** d_white) {
    if (!o) return fail(MW_EINVAL, "NULL handle");
    if (o->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, "mw_ocean_frame_textures: OceanRenderer semantics only");
    const OrState& s = o->orr;
    if (s.frames_last < 1) return fail(MW_ESTATE, "mw_ocean_frame_textures: no mw_ocean_generate_texture_steps_device call yet");
    if (frame < 0 || frame >= s.frames_last) return fail(MW_EINVAL, "mw_ocean_frame_textures: frame out of range");
    const OrFrame f = or_frame(s, frame);
    store_ptrs({d_height, d_disp_xz, d_normal_xyz, d_white}, {f.height, f.disp, f.normal, f.white});  // (disp: (x, z) float pairs)
    return MW_OK;
}

mw_status mw_host_register(void* ptr, size_t bytes) {
    if (!ptr || bytes == 0) return fail(MW_EINVAL, "mw_host_register: NULL pointer or zero size");
    HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterDefault));
    return MW_OK;
}
mw_status mw_host_unregister(void* ptr) {
    if (!ptr) return fail(MW_EINVAL, "mw_host_unregister: NULL pointer");
    HIP_TRY(hipHostUnregister(ptr));
    return MW_OK;
}

mw_status mw_ocean_displace_mesh_device(mw_ocean* o, void* d_vertices_xyz, void* d_normals_xyz, void* d_colors) {
    if (!o || !d_vertices_xyz) return fail(MW_EINVAL, "mw_ocean_displace_mesh: NULL argument");
    if (o->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, "mw_ocean_displace_mesh: OceanRenderer semantics only");
    HIP_TRY(hipSetDevice(o->device));
    return or_displace_mesh(o->orr, o->p.resolution, o->p.unit_width, (float*)d_vertices_xyz, (float*)d_normals_xyz, (float*)d_colors, o->stream);
}

mw_status mw_ocean_displace_mesh(mw_ocean* o, float* vertices_xyz, float* normals_xyz, float* colors) {
    if (!o || !vertices_xyz) return fail(MW_EINVAL, "mw_ocean_displace_mesh: NULL argument");
    if (o->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, "mw_ocean_displace_mesh: OceanRenderer semantics only");
    HIP_TRY(hipSetDevice(o->device));
    const size_t nv = (size_t)o->p.resolution * o->p.resolution * o->orr.tiles;
    void *dv, *dn, *dc;
    Stage<3> st(o);
    st.out(&dv, vertices_xyz, nv * 3 * sizeof(float));
    st.out(&dn, normals_xyz, nv * 3 * sizeof(float));
    st.out(&dc, colors, nv * sizeof(float));
    mw_status s = st.begin();
    if (s != MW_OK) return s;
    if ((s = mw_ocean_displace_mesh_device(o, dv, dn, dc)) != MW_OK) return s;
    return st.finish();
}

// ---- surface services: queries, velocity, hull forces, floating bodies, raycasts ----------------------------------
#include "surface_services.inc"

#include "debug_hooks.inc"  // measurement and test hooks: the profiling hook, mw_debug_* and their kernels
#include "tiles.inc"
#include "pond_host.inc"  // the handle-less Gerstner and pond entry points

}  // extern "C"
