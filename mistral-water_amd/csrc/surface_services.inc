// surface_services.inc -- the host code of the services that read the displaced surface: surface queries, surface velocity, hull
// forces, floating bodies, moorings, mixed fleets, rigged fleets, raycasts, the water column.  Included by mistral_water.hip inside its extern "C" block
// (one translation unit: the handle, fail, HIP_TRY, dmalloc, grow_reserve, Stage / Arr and the frame record are file-static there).
//
// Every service with a host and a device form is a call record and two functions that run it, service_host and service_device below.
// The exported entry points only construct the record.  A record supplies
//   Plan                      what prepare derives from the call and the handle (the mesh of the queried frame, coefficients, ...);
//   prepare(o, frame, who, &plan)   every check either form makes, argument rules first and the handle's state rules last;
//   count()                   the points or bodies of the call: 0 is an empty call, which returns after prepare;
//   check_host(who)           the checks only a host form can make (it reads the caller's arrays);
//   arrays()                  its arrays, declared once (Arr): from this list the device form makes its alignment test and the host form
//                             its Stage, which swaps the staged copies into the record;
//   launch(o, plan)           the kernels, on the handle's stream, on the record's pointers.
// The point services (queries, raycasts, the column query) are PointCall and a struct each; the hull family (hull forces, step bodies,
// step moored) is one HullCall whose optional parts say which call it is; the fleets (step rigged included) are one FleetCall.  The per-substep plan of all
// stepping is run_substeps, the raycasts' hierarchy raycast_tree.  mw_ocean_velocity / _device have no arrays to stage and stand alone.

static int sq_iters(int32_t iterations) { return iterations == 0 ? MW_SQ_DEFAULT_ITERS : iterations; }
// device entry points: p is not a multiple of `bytes` (a power of two)
static bool misaligned(const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) != 0; }
static bool triangles_in_range(const void* triangles, int32_t ntris, int32_t nverts) {
    const int32_t* t = static_cast<const int32_t*>(triangles);
    for (int64_t k = 0; k < (int64_t)ntris * 3; k++)
        if (t[k] < 0 || t[k] >= nverts) return false;
    return true;
}
static void* vp(const void* p) { return const_cast<void*>(p); }  // a call record keeps every array pointer as void* (Arr::slot)
// the handle has one surface to read: not NULL, not a batch of tiles
static mw_status single_surface_check(const mw_ocean* o, const char* who) {
    if (!o) return fail(MW_EINVAL, who, "NULL handle");
    if (o->sem == MW_SEM_OCEANRENDERER && o->orr.tiles != 1)
        return fail(MW_EINVAL, who, "a batched handle (mw_ocean_create_batch) has no single surface");
    return MW_OK;
}

extern "C++" {  // templates stand outside C linkage
// The host form of a service: validate, return on an empty call, the host-only checks, stage the arrays, launch on the copies, copy back
// and wait for the stream.
template <class Call>
static mw_status service_host(mw_ocean* o, int32_t frame, const Call& c, const char* who) {
    if (o) HIP_TRY(hipSetDevice(o->device));
    typename Call::Plan p{};
    mw_status s = c.prepare(o, frame, who, &p);
    if (s != MW_OK || c.count() == 0) return s;
    if ((s = c.check_host(who)) != MW_OK) return s;
    Call d = c;  // the same call on the staged copies
    Stage st(o, d.arrays());
    if ((s = st.begin()) != MW_OK || (s = d.launch(o, p)) != MW_OK) return s;
    return st.finish();
}
// The device form: the alignment of the caller's arrays (before the handle is looked at; `aligned` is the entry point's own message),
// validate, return on an empty call, launch.  Never waits for the stream.
template <class Call>
static mw_status service_device(mw_ocean* o, int32_t frame, Call c, const char* who, const char* aligned) {
    if (o) HIP_TRY(hipSetDevice(o->device));
    if (c.count() > 0)
        for (const Arr& a : c.arrays())
            if (misaligned(*a.slot, a.align)) return fail(MW_EINVAL, who, aligned);
    typename Call::Plan p{};
    mw_status s = c.prepare(o, frame, who, &p);
    if (s != MW_OK || c.count() == 0) return s;
    return c.launch(o, p);
}
}  // extern "C++"

// The arguments of a point service: n points (or rays) in, n rows out, and for the raycasts the optional hit record per ray.  The host and
// the device form differ only in whose pointers it holds; each service below adds its prepare, arrays and launch.
namespace {
struct PointCall {
    using Plan = SqMesh;
    void *pts, *out, *hit;
    int64_t n; int32_t mode, iterations, reach;
    int64_t count() const { return n; }
    mw_status check_host(const char*) const { return MW_OK; }
    size_t floats(int per) const { return (size_t)n * per * sizeof(float); }  // bytes of n rows of `per` 4-byte words
};
}  // namespace

// ---- surface queries (csrc/surface_query.h) -------------------------------------------------------------------
// Validates the call and names the vertex arrays of the queried frame.  OceanRenderer: the material's vertex stage of that frame
// (k_or_displace_mesh, so the vertices are those of mw_ocean_displace_mesh bit for bit) runs into the handle's q_mesh first.
// This is the one place an SqMesh is filled: a periodic handle (mw_ocean_set_periodic) gets its period here, every other mesh 0, and the
// launches below pick the kernels' SqTiled instantiations (surface_tiled.h) from m.period != 0.
// the argument rules of a point query that need no handle (mw_debug_query_mesh, debug_hooks.inc, applies them to a caller's mesh)
static mw_status query_args_check(int32_t mode, const void* xz, int64_t n, int32_t iterations, const void* out, const char* who) {
    if (n < 0) return fail(MW_EINVAL, who, "n < 0");
    if (n > 0 && (!xz || !out)) return fail(MW_EINVAL, who, "NULL array");
    if (mode != MW_QUERY_REST && mode != MW_QUERY_WORLD) return fail(MW_EINVAL, who, "mode must be MW_QUERY_REST or MW_QUERY_WORLD");
    if (iterations < 0 || iterations > MW_SQ_MAX_ITERS) return fail(MW_EINVAL, who, "iterations must be in [0,64]");
    // one launch: gridDim.x * blockDim.x must fit in 32 bits
    if (n > (int64_t)UINT32_MAX - 255) return fail(MW_EINVAL, who, "n > 2^32 - 256 (one launch)");
    return MW_OK;
}
// The launches of the two point queries, one lane per point in blocks of 256: the services below and mw_debug_query_mesh both launch here,
// so the hook runs the services' grid rule, iterations mapping and kernel instantiations.
static mw_status query_surface_launch(hipStream_t st, const SqMesh& m, int32_t mode, int32_t iterations, const void* pts, int64_t n, void* out) {
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    const float2* xz = static_cast<const float2*>(pts);
    if (m.period != 0.f) HIP_TRY(tiled_query_surface(grid, st, m, mode, sq_iters(iterations), xz, n, static_cast<float4*>(out)));
    else k_query_surface<<<grid, block, 0, st>>>(m, mode, sq_iters(iterations), xz, n, static_cast<float4*>(out));
    HIP_TRY(hipGetLastError());
    return MW_OK;
}
static mw_status query_velocity_launch(hipStream_t st, const SqMesh& m, const float* vel, int32_t mode, int32_t iterations, const void* pts,
                                       int64_t n, void* out) {
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    const float2* xz = static_cast<const float2*>(pts);
    if (m.period != 0.f) HIP_TRY(tiled_query_velocity(grid, st, m, vel, mode, sq_iters(iterations), xz, n, static_cast<float4*>(out)));
    else k_query_velocity<<<grid, block, 0, st>>>(m, vel, mode, sq_iters(iterations), xz, n, static_cast<float4*>(out));
    HIP_TRY(hipGetLastError());
    return MW_OK;
}
static mw_status query_prepare(mw_ocean* o, int32_t frame, int32_t mode, const void* xz, int64_t n, int32_t iterations, const void* out,
                               const char* who, SqMesh* m) {
    if (!o) return fail(MW_EINVAL, who, "NULL handle");
    const mw_status args = query_args_check(mode, xz, n, iterations, out, who);
    if (args != MW_OK) return args;
    if (o->sem == MW_SEM_OCEANRENDERER && o->orr.tiles != 1)
        return fail(MW_EINVAL, who, "a batched handle (mw_ocean_create_batch) has no single surface");
    if (o->sem == MW_SEM_FFTMESH && frame != -1) return fail(MW_EINVAL, who, "FFTMesh handles keep one frame (frame = -1)");
    if (o->sem == MW_SEM_OCEANRENDERER && (frame < -1 || (frame >= 0 && frame >= o->orr.frames_last)))
        return fail(MW_EINVAL, who, "frame out of range (-1, or a frame of the latest steps call)");
    if (!(o->p.unit_width > 0.f)) return fail(MW_EINVAL, who, "the mesh needs unit_width > 0");
    m->unit_width = o->p.unit_width;
    m->period = o->periodic ? grid_period(o) : 0.f;
    if (o->sem == MW_SEM_FFTMESH) {
        if (!o->fm.s_have) return fail(MW_ESTATE, who, "no frame yet (mw_ocean_evaluate / mw_ocean_update first)");
        m->vert = o->fm.s_vert; m->norm = o->fm.s_norm; m->white = o->fm.s_white; m->R = o->N; m->wstride = o->fm.s_wstride;
        return MW_OK;
    }
    OrState& r = o->orr;
    if (frame == -1 && !r.have_frame) return fail(MW_ESTATE, who, "no GenerateTexture() yet");
    const OrFrame f = or_frame(r, frame);
    if (!f.complete) return fail(MW_ESTATE, who, "the steps call sent this frame's textures to caller buffers");
    const int res = o->p.resolution, nv = res * res;
    if (n == 0) return MW_OK;
    if (!o->q_mesh) {
        mw_status s = dmalloc(&o->q_mesh, (size_t)nv * 7);
        if (s != MW_OK) return s;
    }
    float *qv = o->q_mesh, *qn = qv + (size_t)nv * 3, *qw = qn + (size_t)nv * 3;
    k_or_displace_mesh<<<dim3((unsigned)((nv + 255) / 256), 1), dim3(256), 0, o->stream>>>(r.M, res, o->p.unit_width, f.height, f.disp, f.normal,
                                                                                          f.white, qv, qn, qw);
    HIP_TRY(hipGetLastError());
    m->vert = qv; m->norm = qn; m->white = qw; m->R = res; m->wstride = 1;
    return MW_OK;
}
namespace {
struct QuerySurface : PointCall {
    mw_status prepare(mw_ocean* o, int32_t frame, const char* who, SqMesh* m) const {
        return query_prepare(o, frame, mode, pts, n, iterations, out, who, m);
    }
    std::array<Arr, 2> arrays() { return {{{&pts, floats(2), IN, 8}, {&out, floats(8), OUT, 16}}}; }
    mw_status launch(mw_ocean* o, const SqMesh& m) const { return query_surface_launch(o->stream, m, mode, iterations, pts, n, out); }
};
}  // namespace

mw_status mw_ocean_query_surface_device(mw_ocean* o, int32_t frame, int32_t mode, const void* d_xz, int64_t n, int32_t iterations,
                                        void* d_out) {
    return service_device(o, frame, QuerySurface{{vp(d_xz), d_out, nullptr, n, mode, iterations, 0}}, "mw_ocean_query_surface_device",
                          "d_xz must be 8-byte and d_out 16-byte aligned");
}
mw_status mw_ocean_query_surface(mw_ocean* o, int32_t frame, int32_t mode, const float* xz, int64_t n, int32_t iterations, float* out) {
    return service_host(o, frame, QuerySurface{{vp(xz), out, nullptr, n, mode, iterations, 0}}, "mw_ocean_query_surface");
}

// ---- surface velocity (csrc/velocity_kernels.h) --------------------------------------------------------------------
// The frame a velocity call differentiates: FFTMesh the latest frame (frame -1); OceanRenderer the current phase, which is the latest
// frame's (-1) or the last frame of the latest steps call while no other call has moved the phase since.  Argument errors first, as
// query_prepare orders them.
static mw_status velocity_check(mw_ocean* o, int32_t frame, const char* who) {
    mw_status s = single_surface_check(o, who);
    if (s != MW_OK) return s;
    if (o->sem == MW_SEM_FFTMESH && frame != -1) return fail(MW_EINVAL, who, "FFTMesh handles keep one frame (frame = -1)");
    if (o->sem == MW_SEM_OCEANRENDERER && frame != -1 && !(frame >= 0 && frame == o->or_steps_tail))
        return fail(MW_EINVAL, who, "the handle keeps only the latest phase: frame must be -1 or the last frame of the latest "
                                    "steps call");
    if (o->sem == MW_SEM_FFTMESH && !o->fm.s_have) return fail(MW_ESTATE, who, "no frame yet (mw_ocean_evaluate / mw_ocean_update first)");
    if (o->sem == MW_SEM_OCEANRENDERER && !o->orr.have_frame) return fail(MW_ESTATE, who, "no GenerateTexture() yet");
    return MW_OK;
}
// the velocity of every vertex into d_vel [R*R][3], on the handle's stream; writes only the handle's velocity buffers
static mw_status velocity_run(mw_ocean* o, float* d_vel) {
    VelState& v = o->vel;
    if (o->sem == MW_SEM_OCEANRENDERER) {
        return or_velocity(o->orr, v, o->p.resolution, d_vel, o->stream);
    }
    const int N = o->N;
    const size_t NN = (size_t)N * N;
    mw_status s = MW_OK;
    if (!v.white) {  // the last buffer allocated: a failure half-way frees them all, and the next call starts again
        if ((s = fm_spectrum_alloc(v.sp, N, o->use_fft)) != MW_OK || (s = dmalloc(&v.norm, 3 * NN)) != MW_OK || (s = dmalloc(&v.white, NN)) != MW_OK) {
            vel_free(v);
            return s;
        }
    }
    const unsigned nb = (unsigned)((NN + 255) / 256);
    if (!v.ready) {  // (i w h0, -i w h0c) and, on the FFT path, its prep tables: once per spectrum
        hipLaunchKernelGGL(k_velocity_spectrum, dim3(nb), dim3(256), 0, o->stream, N, o->p.length, o->p.gravity, o->fm.sp.h0, o->fm.sp.h0c, v.sp.h0,
                           v.sp.h0c);
        HIP_TRY(hipGetLastError());
        if (o->use_fft && (s = fm_prep(v.sp, N, o->p.length, o->p.gravity, o->fm.Wpre, o->stream)) != MW_OK) return s;
        velocity_spectrum_built(o);
    }
    OceanConsts C = consts_of(o);
    C.choppiness = o->fm.s_chop;  // the frame's choppiness (mw_ocean_set_choppiness may have changed it since)
    if (!o->use_fft) {
        if ((s = direct_evaluate(o->direct, C, v.sp.h0, v.sp.h0c, o->fm.s_t, d_vel, v.norm, v.white, 1, o->stream)) != MW_OK) return s;
        hipLaunchKernelGGL(k_velocity_from_hds, dim3(nb), dim3(256), 0, o->stream, N, C.choppiness, o->direct.hds, d_vel);
        HIP_TRY(hipGetLastError());
        return MW_OK;
    }
    // pass 2 around a rest coordinate of +-0 (unit_width = 0): the vertex the epilogue writes is (-chop Dx, h, -chop Dz) of the weighted spectrum
    return fm_evaluate(o->fm, v.sp, C, &o->fm.s_t, 1, d_vel, v.norm, v.white, 1, o->stream, true);
}
static size_t velocity_count(const mw_ocean* o) {  // floats of the per-vertex velocity [R*R][3]
    const int R = o->sem == MW_SEM_OCEANRENDERER ? o->p.resolution : o->N;
    return (size_t)R * R * 3;
}
// the velocity of every vertex into the handle's own buffer o->vel.vert (allocated on first use)
static mw_status velocity_to_handle(mw_ocean* o) {
    mw_status s = o->vel.vert ? MW_OK : dmalloc(&o->vel.vert, velocity_count(o));
    return s != MW_OK ? s : velocity_run(o, o->vel.vert);
}

mw_status mw_ocean_velocity_device(mw_ocean* o, int32_t frame, void* d_velocity_xyz) {
    const char* who = "mw_ocean_velocity_device";
    mw_status s = velocity_check(o, frame, who);
    if (s != MW_OK) return s;
    if (!d_velocity_xyz) return fail(MW_EINVAL, who, "NULL array");
    HIP_TRY(hipSetDevice(o->device));
    return velocity_run(o, static_cast<float*>(d_velocity_xyz));
}

mw_status mw_ocean_velocity(mw_ocean* o, int32_t frame, float* velocity_xyz) {
    const char* who = "mw_ocean_velocity";
    mw_status s = velocity_check(o, frame, who);
    if (s != MW_OK) return s;
    if (!velocity_xyz) return fail(MW_EINVAL, who, "NULL array");
    HIP_TRY(hipSetDevice(o->device));
    if ((s = velocity_to_handle(o)) != MW_OK) return s;
    HIP_TRY(hipMemcpyAsync(velocity_xyz, o->vel.vert, velocity_count(o) * sizeof(float), hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(hipStreamSynchronize(o->stream));
    return MW_OK;
}

// velocity queries: the surface query's validation and mesh (query_prepare), the per-vertex velocity into the handle's buffer, one lane
// per point locating exactly as k_query_surface does (sq_locate)
// The located surface is the latest frame's; the velocity is that of the handle's current spectrum and phase.  Once either moved on
// without a new frame (mw_ocean_set_spectrum / reinit_spectrum / set_phase / advance_phase) the two would belong to different
// instants: MW_ESTATE until the next frame.
static mw_status query_velocity_prepare(mw_ocean* o, int32_t frame, int32_t mode, const void* xz, int64_t n, int32_t iterations, const void* out,
                                        const char* who, SqMesh* m) {
    mw_status s = query_prepare(o, frame, mode, xz, n, iterations, out, who, m);
    if (s == MW_OK) s = velocity_check(o, frame, who);
    if (s == MW_OK && o->frame_behind)
        return fail(MW_ESTATE, who, "the spectrum or phase changed after the latest frame: the surface and the velocity would "
                                    "belong to different instants (make a frame first)");
    return s;
}
namespace {
struct QueryVelocity : PointCall {
    mw_status prepare(mw_ocean* o, int32_t frame, const char* who, SqMesh* m) const {
        return query_velocity_prepare(o, frame, mode, pts, n, iterations, out, who, m);
    }
    std::array<Arr, 2> arrays() { return {{{&pts, floats(2), IN, 8}, {&out, floats(4), OUT, 16}}}; }
    mw_status launch(mw_ocean* o, const SqMesh& m) const {
        mw_status s = velocity_to_handle(o);
        return s != MW_OK ? s : query_velocity_launch(o->stream, m, o->vel.vert, mode, iterations, pts, n, out);
    }
};
}  // namespace

mw_status mw_ocean_query_velocity_device(mw_ocean* o, int32_t frame, int32_t mode, const void* d_xz, int64_t n, int32_t iterations, void* d_out) {
    return service_device(o, frame, QueryVelocity{{vp(d_xz), d_out, nullptr, n, mode, iterations, 0}}, "mw_ocean_query_velocity_device",
                          "d_xz must be 8-byte and d_out 16-byte aligned");
}
mw_status mw_ocean_query_velocity(mw_ocean* o, int32_t frame, int32_t mode, const float* xz, int64_t n, int32_t iterations, float* out) {
    return service_host(o, frame, QueryVelocity{{vp(xz), out, nullptr, n, mode, iterations, 0}}, "mw_ocean_query_velocity");
}

// ---- hull forces (csrc/hull_forces.h) -----------------------------------------------------------------------------
// The arguments of a hull-family call.  The host and the device form of an entry point differ only in which pointers it holds: the
// caller's own (prepare reads none of them but the host-side coeffs), or their staged copies (launch).  Its optional parts say which
// call it is.  step (mw_ocean_step_bodies): mass is required, bodies are updated in place, out is optional, dt and substeps are read.
// moored (mw_ocean_step_moored, a stepping call): lines, K = lines_per_body and the optional tension.
struct HullCall {
    void *hull, *tris, *bodies, *out;
    int32_t nverts, ntris, nbodies, iterations; const float* coeffs;
    bool step; void* mass; float dt; int32_t substeps;
    bool moored; void* lines; int32_t K; void* tension;
};
// what prepare derives from the call and the handle: the mesh of the queried frame and the coefficients as the kernels take them
struct HullPlan { SqMesh m; HullCoeffs cf; float vscale, g; };  // vscale = coeffs[4]; g = coeffs[1], gravity (step bodies)

// the water column's host code (below), as the hull family calls it with draught on (mw_ocean_set_draught, csrc/hull_draught.h)
static mw_status column_prepare(mw_ocean* o, int32_t frame, int32_t mode, const void* xyz, int64_t n, int32_t iterations, const void* out,
                                const char* who, SqMesh* m);
static mw_status column_build(mw_ocean* o);
static ColTable column_table(const mw_ocean* o, const SqMesh& m);

// Validates a hull-forces call and names the surface it reads: the surface query's rules and mesh (query_prepare) with drag off, the
// velocity query's (query_velocity_prepare: frame rules of the velocity, MW_ESTATE once the spectrum or phase moved on) with drag on.
// With draught on, drag on or off, the column's (column_prepare: the same mesh, MW_ESTATE without a column or once the spectrum or phase
// moved on) after the call's own argument checks.
static mw_status hull_prepare(mw_ocean* o, int32_t frame, const HullCall& c, const char* who, HullPlan* p) {
    mw_status s = single_surface_check(o, who);
    if (s != MW_OK) return s;
    if (c.nbodies < 0) return fail(MW_EINVAL, who, "nbodies < 0");
    if (c.nverts < 3 || c.ntris < 1) return fail(MW_EINVAL, who, "a hull needs nverts >= 3 and ntris >= 1");
    if (!c.coeffs) return fail(MW_EINVAL, who, "NULL coeffs");
    if (c.nbodies > 0 && (!c.hull || !c.tris || !c.bodies || !c.out)) return fail(MW_EINVAL, who, "NULL array");
    const int64_t lim = ((int64_t)1 << 31) - 256;
    if ((int64_t)c.nbodies * c.nverts > lim || (int64_t)c.nbodies * c.ntris > lim)
        return fail(MW_EINVAL, who, "nbodies * nverts and nbodies * ntris must not exceed 2^31 - 256");
    for (int k = 0; k < MW_HULL_NCOEFFS; k++)
        if (!(c.coeffs[k] >= 0.f && c.coeffs[k] <= 3.4e38f)) return fail(MW_EINVAL, who, "coefficients must be finite and >= 0");
    hull_coeffs(c.coeffs, &p->cf, &p->g, &p->vscale);
    // the surface (and, with drag on, the velocity) of the frame; the markers stand for the query's arrays, checked above
    const void* mark = c.nbodies > 0 ? c.bodies : nullptr;
    if (o->draught) return column_prepare(o, frame, MW_QUERY_WORLD, mark, c.nbodies, c.iterations, mark, who, &p->m);
    return p->cf.drag ? query_velocity_prepare(o, frame, MW_QUERY_WORLD, mark, c.nbodies, c.iterations, mark, who, &p->m)
                      : query_prepare(o, frame, MW_QUERY_WORLD, mark, c.nbodies, c.iterations, mark, who, &p->m);
}
static int hull_chunks(const HullCall& c) { return hull_chunks(c.nverts, c.ntris); }
// the kernels' view of a call on device pointers; vslab, part and out are the launch's own (hull_launch)
static HullArgs hull_args(const mw_ocean* o, const HullPlan& p, const HullCall& c) {
    HullArgs a{};
    a.m = p.m;
    a.vel = p.cf.drag ? o->vel.vert : nullptr;
    a.vscale = p.vscale;
    a.iters = sq_iters(c.iterations);
    a.cf = p.cf;
    a.hull = static_cast<const float*>(c.hull); a.tris = static_cast<const int32_t*>(c.tris); a.bodies = static_cast<const float4*>(c.bodies);
    a.nverts = c.nverts; a.ntris = c.ntris; a.nchunks = hull_chunks(c); a.nbodies = c.nbodies;
    return a;
}
// The work space of the three hull kernels over nv instance vertices, nblk (body, chunk) items and nb bodies, for hull_launch and
// fleet_rows: the vertex slab and, 256-byte aligned behind it, the chunk partials in the handle's grow-only buffer, and the three grids
struct HullWork { float4 *vslab, *part; dim3 gv, gt, gr; };
static mw_status hull_reserve(mw_ocean* o, int64_t nv, int64_t nblk, int64_t nb, HullWork* w) {
    const size_t bslab = align256((size_t)nv * 8 * sizeof(float)), bpart = (size_t)nblk * 8 * sizeof(float);
    mw_status s = grow_reserve(o, o->hull, bslab + bpart, "the hull-forces buffer");
    if (s != MW_OK) return s;
    w->vslab = static_cast<float4*>(o->hull.p);
    w->part = reinterpret_cast<float4*>(static_cast<char*>(o->hull.p) + bslab);
    w->gv = dim3((unsigned)((nv + 255) / 256));
    w->gt = dim3((unsigned)std::min<int64_t>(nblk, (int64_t)1 << 20));
    w->gr = dim3((unsigned)std::min<int64_t>((nb + 3) / 4, (int64_t)1 << 20));
    return MW_OK;
}
// The water a hull call reads, made current once per frame: with draught on the layers (column_build, whether or not drag is on: it
// makes layer 0's velocity current too), otherwise with drag on the velocity field in o->vel.vert.
static mw_status hull_water(mw_ocean* o, const HullPlan& p) {
    if (o->draught) return column_build(o);
    return p.cf.drag ? velocity_to_handle(o) : MW_OK;
}
// The kernels after the vertex slab exist once per rounding mode (hull_forces.h): the strict build (surface_tiled.hip) serves draught
// and the periodic handle, mistral_water.hip's contracted one the one footprint without draught.
static bool hull_strict(const mw_ocean* o, const SqMesh& m) { return o->draught || m.period != 0.f; }
// the three launches on the handle's stream (nbodies > 0), the rows into c.out: the vertex phase, chosen by (draught, period), then
// the rows (k_hull_triangles, k_hull_reduce), chosen by hull_strict
// velocity = false: the water is current already (mw_ocean_step_bodies sees to it once per call)
static mw_status hull_launch(mw_ocean* o, const HullPlan& p, const HullCall& c, bool velocity = true) {
    HullWork w;
    mw_status s = hull_reserve(o, (int64_t)c.nbodies * c.nverts, (int64_t)c.nbodies * hull_chunks(c), c.nbodies, &w);
    if (s != MW_OK) return s;
    if (velocity && (s = hull_water(o, p)) != MW_OK) return s;
    HullArgs a = hull_args(o, p, c);
    a.vslab = w.vslab;
    a.part = w.part;
    a.out = static_cast<float4*>(c.out);
    if (o->draught) HIP_TRY(draught_vertices_launch(o->stream, w.gv, a, column_table(o, p.m)));
    else if (a.m.period != 0.f) HIP_TRY(tiled_hull_vertices(w.gv, o->stream, a));
    else k_hull_vertices<<<w.gv, dim3(256), 0, o->stream>>>(a);
    if (hull_strict(o, a.m)) {
        HIP_TRY(strict_hull_rows(w.gt, w.gr, o->stream, a));
    } else {
        k_hull_triangles<<<w.gt, dim3(MW_HULL_CHUNK), 0, o->stream>>>(a);
        k_hull_reduce<<<w.gr, dim3(256), 0, o->stream>>>(a);
        HIP_TRY(hipGetLastError());
    }
    return MW_OK;
}

// ---- floating bodies (csrc/rigid_bodies.h) ------------------------------------------------------------------------
static_assert(MW_BODY_NMASS == 8, "rigid_bodies.h reads 8 floats per mass row");

mw_status mw_hull_mass_properties(const float* hull_xyz, int32_t nverts, const int32_t* triangles, int32_t ntris, float density,
                                  float* out) {
    const char* who = "mw_hull_mass_properties";
    if (!hull_xyz || !triangles || !out) return fail(MW_EINVAL, who, "NULL array");
    if (nverts < 3 || ntris < 1) return fail(MW_EINVAL, who, "a hull needs nverts >= 3 and ntris >= 1");
    if (!(density > 0.f && density <= 3.4e38f)) return fail(MW_EINVAL, who, "density must be finite and > 0");
    if (!triangles_in_range(triangles, ntris, nverts)) return fail(MW_EINVAL, who, "triangle index outside [0, nverts)");
    // signed tetrahedra from the vertex mean o (conditioning): volume, first and second moments, all f64
    double o3[3] = {0.0, 0.0, 0.0};
    for (int v = 0; v < nverts; v++)
        for (int c = 0; c < 3; c++) o3[c] += hull_xyz[3 * v + c];
    for (int c = 0; c < 3; c++) o3[c] /= nverts;
    double V = 0.0, M1[3] = {0.0, 0.0, 0.0}, M2[3][3] = {{0.0}};
    for (int t = 0; t < ntris; t++) {
        double p[3][3], s[3];
        for (int i = 0; i < 3; i++)
            for (int c = 0; c < 3; c++) p[i][c] = (double)hull_xyz[3 * triangles[3 * t + i] + c] - o3[c];
        const double vt = (p[0][0] * (p[1][1] * p[2][2] - p[1][2] * p[2][1]) - p[0][1] * (p[1][0] * p[2][2] - p[1][2] * p[2][0]) +
                           p[0][2] * (p[1][0] * p[2][1] - p[1][1] * p[2][0])) / 6.0;
        for (int c = 0; c < 3; c++) s[c] = p[0][c] + p[1][c] + p[2][c];
        V += vt;
        for (int c = 0; c < 3; c++) M1[c] += vt * s[c] / 4.0;
        // int x_i x_j over the tetrahedron (0, a, b, c) = V / 20 (sum_k a_i a_j + s_i s_j)
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++)
                M2[i][j] += vt / 20.0 * (p[0][i] * p[0][j] + p[1][i] * p[1][j] + p[2][i] * p[2][j] + s[i] * s[j]);
    }
    if (!(V > 0.0) || !std::isfinite(V)) return fail(MW_EINVAL, who, "the hull's volume is not positive (an open or inward-wound mesh)");
    double cen[3], C[3][3];
    for (int c = 0; c < 3; c++) cen[c] = M1[c] / V;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) C[i][j] = density * (M2[i][j] - V * cen[i] * cen[j]);  // int x_i x_j dm about the centroid
    out[0] = (float)(density * V);
    for (int c = 0; c < 3; c++) out[1 + c] = (float)(cen[c] + o3[c]);
    out[4] = (float)(C[1][1] + C[2][2]);
    out[5] = (float)(C[0][0] + C[2][2]);
    out[6] = (float)(C[0][0] + C[1][1]);
    out[7] = (float)(-C[0][1]);
    out[8] = (float)(-C[0][2]);
    out[9] = (float)(-C[1][2]);
    return MW_OK;
}

// Validates a step-bodies call: its own arguments, then the hull-forces rules (hull_prepare; out is optional here, so the bodies stand
// in for it).
static mw_status bodies_prepare(mw_ocean* o, int32_t frame, const HullCall& c, const char* who, HullPlan* p) {
    if (!(c.substeps >= 1 && c.substeps <= 64)) return fail(MW_EINVAL, who, "substeps must be in [1, 64]");
    if (!(c.dt >= 0.f && c.dt <= 3.4e38f)) return fail(MW_EINVAL, who, "dt must be finite and >= 0");
    if (c.nbodies > 0 && !c.mass) return fail(MW_EINVAL, who, "NULL array");
    HullCall h = c;
    h.out = c.bodies;
    return hull_prepare(o, frame, h, who, p);
}

// The plan rule (MW_BODIES_PLAN = -1), DESIGN.md section 7e: one launch for hulls of at most 3 chunks (768 triangles and vertices),
// per substep above.  Measured: 1024 icospheres (2 chunks) 0.49x the per-substep time; 64 barges (22 chunks) 1.8x.
static bool bodies_one_launch_rule(int nchunks) { return nchunks < 4; }
// a hull steps in one launch (k_bodies_step on the one footprint, k_fleet_step on a periodic handle): its slab and partials fit in LDS, and the switch asks for it or the rule does
static bool bodies_one_launch(int nverts, int nchunks) {
    const int plan = sw(SW_BODIES_PLAN);
    return bodies_step_lds(nverts, nchunks) <= MW_BODIES_LDS_MAX && (plan == 1 || (plan < 0 && bodies_one_launch_rule(nchunks)));
}
// row b of a host array of mass rows, as both host forms of stepping check and report it
static mw_status mass_row_check(const void* mass, int32_t b, const char* who) {
    if (body_mass_valid(static_cast<const float*>(mass) + 8 * (size_t)b)) return MW_OK;
    return fail(MW_EINVAL, who, "the mass row of body " + std::to_string(b) +
                                    " is invalid (m <= 0 or not finite, or I_b not positive definite)");
}

// the kernels' view of a stepping call on device pointers; rows and last are the per-substep plan's own (run_substeps)
static BodiesArgs bodies_args(const mw_ocean* o, const HullPlan& p, const HullCall& c) {
    BodiesArgs a{};
    a.h = hull_args(o, p, c);
    a.bodies = static_cast<float4*>(c.bodies);
    a.mass = static_cast<const float4*>(c.mass);
    a.out = static_cast<float4*>(c.out);
    a.g = p.g;
    a.dt = c.dt / (float)c.substeps;
    a.substeps = c.substeps;
    return a;
}
// The call as a one-hull fleet table with the plan's coefficients: what the strict one-launch kernel shared with the fleets reads (fleet.h)
static FleetTable hull_table(const HullPlan& p, const HullCall& c) {
    const int32_t one[MW_FLEET_NHULL] = {0, c.nverts, 0, c.ntris, c.nbodies};
    FleetTable t{};
    fleet_table(one, 1, 1u, &t);
    t.hull[0].cf = p.cf; t.hull[0].g = p.g; t.hull[0].vscale = p.vscale;
    return t;
}
// The one-launch plan of a single-hull stepping call on a periodic handle: k_fleet_step over the call's one-hull table, without a
// wrench, with the call's lines when it is moored (K == 0 otherwise)
static mw_status hull_step_launch(mw_ocean* o, const HullPlan& p, const HullCall& c) {
    const HullArgs h = hull_args(o, p, c);  // the surface, the velocity rule and the geometry are the hull call's
    FleetArgs a{};
    a.m = h.m; a.vel = h.vel; a.iters = h.iters; a.hull = h.hull; a.tris = h.tris;
    a.bodies = static_cast<float4*>(c.bodies);
    a.mass = static_cast<const float4*>(c.mass);
    a.out = static_cast<float4*>(c.out);
    a.dt = c.dt / (float)c.substeps;
    a.substeps = c.substeps;
    a.t = hull_table(p, c);
    HIP_TRY(tiled_fleet_step(dim3((unsigned)c.nbodies), bodies_step_lds(c.nverts, hull_chunks(c)), MW_BODIES_LDS_MAX, o->stream, a,
                             static_cast<const float4*>(c.lines), c.K, static_cast<float*>(c.tension)));
    return MW_OK;
}
extern "C++" {
// The per-substep plan of every stepping call, on the handle's stream: the handle's row buffer holds nrows rows; per substep rows(buf)
// launches the hull forces of the bodies' current state into it and integrate(buf, last) steps the bodies by them, last on the final
// substep (the one whose rows go to the caller's out).
template <class Rows, class Integrate>
static mw_status run_substeps(mw_ocean* o, int64_t nrows, int substeps, Rows rows, Integrate integrate) {
    mw_status s = grow_reserve(o, o->bodies, (size_t)nrows * 8 * sizeof(float), "the step-bodies row buffer");
    if (s != MW_OK) return s;
    float4* buf = static_cast<float4*>(o->bodies.p);
    for (int k = 0; k < substeps; k++)
        if ((s = rows(buf)) != MW_OK || (s = integrate(buf, k == substeps - 1)) != MW_OK) return s;
    return MW_OK;
}
}  // extern "C++"

// every substep of the call on the handle's stream (nbodies > 0): the water once (hull_water: the surface is frozen for the call), then
// one launch (k_fleet_step on a periodic handle, hull_step_launch; the contracted k_bodies_step on the one footprint), or per substep
// hull_launch and k_bodies_integrate, the strict build where hull_launch's rows are (hull_strict).  Draught on: there is no one-launch
// plan on the column and MW_BODIES_PLAN is not read.
static mw_status bodies_launch(mw_ocean* o, const HullPlan& p, const HullCall& c) {
    const int nchunks = hull_chunks(c);
    mw_status s = hull_water(o, p);
    if (s != MW_OK) return s;
    BodiesArgs a = bodies_args(o, p, c);
    if (!o->draught && bodies_one_launch(c.nverts, nchunks)) {
        if (p.m.period != 0.f) return hull_step_launch(o, p, c);
        static AttrOnce attr;
        HIP_TRY(attr.set(reinterpret_cast<const void*>(k_bodies_step<SqMesh>), MW_BODIES_LDS_MAX));
        k_bodies_step<<<dim3((unsigned)c.nbodies), dim3(MW_HULL_CHUNK), bodies_step_lds(c.nverts, nchunks), o->stream>>>(a);
        HIP_TRY(hipGetLastError());
        return MW_OK;
    }
    HullCall rows = c;  // the hull forces of a substep: the same call, its rows into the handle's buffer
    const dim3 gi((unsigned)(((int64_t)c.nbodies + 255) / 256));
    return run_substeps(
        o, c.nbodies, c.substeps, [&](float4* buf) { rows.out = buf; return hull_launch(o, p, rows, false); },
        [&](const float4* buf, bool last) -> mw_status {
            a.rows = buf;
            a.last = last;
            if (hull_strict(o, a.h.m)) HIP_TRY(strict_bodies_integrate(gi, o->stream, a));
            else k_bodies_integrate<<<gi, dim3(256), 0, o->stream>>>(a);
            HIP_TRY(hipGetLastError());
            return MW_OK;
        });
}

// ---- moorings (csrc/moorings.h) -----------------------------------------------------------------------------------
static_assert(MW_MOORING_MAX_LINES == MW_MOORING_LINES && MW_MOORING_NLINE == MW_MOORING_SLOT, "moorings.h and the ABI size a slot alike");

// Validates a step-moored call: its own arguments, then the step-bodies rules (bodies_prepare).
static mw_status moored_prepare(mw_ocean* o, int32_t frame, const HullCall& c, const char* who, HullPlan* p) {
    if (c.K < 1 || c.K > MW_MOORING_MAX_LINES) return fail(MW_EINVAL, who, "lines_per_body must be in [1, MW_MOORING_MAX_LINES]");
    if (c.nbodies > 0 && !c.lines) return fail(MW_EINVAL, who, "NULL lines");
    return bodies_prepare(o, frame, c, who, p);
}
// The one-launch plan takes the hull when step bodies would (bodies_one_launch) and the slots and tensions fit beside its slab in the
// 1 KiB MW_BODIES_LDS_MAX leaves free.  A plan rule, not a fit rule: k_fleet_step holds that LDS for every call, so the launch would
// fit up to step bodies' own edge; the rule keeps the plan of every hull size where it was (the edge at 5055 / 5056 vertices).
static bool moored_one_launch(int nverts, int nchunks) {
    return bodies_one_launch(nverts, nchunks) && bodies_step_lds(nverts, nchunks) + MW_MOORED_LDS_STATIC <= MW_BODIES_LDS_MAX;
}
// every substep of the call on the handle's stream (nbodies > 0), as bodies_launch: the water once, then one k_fleet_step launch with
// the lines (hull_step_launch: a periodic handle without draught whose hull qualifies; MW_BODIES_PLAN is honoured) or per substep
// hull_launch and k_moored_integrate.  A non-periodic handle and draught always step per substep, as the fleets and draught do.
static mw_status moored_launch(mw_ocean* o, const HullPlan& p, const HullCall& c) {
    mw_status s = hull_water(o, p);
    if (s != MW_OK) return s;
    if (!o->draught && p.m.period != 0.f && moored_one_launch(c.nverts, hull_chunks(c))) return hull_step_launch(o, p, c);
    MooredArgs a{};
    a.bodies = static_cast<float4*>(c.bodies);
    a.mass = static_cast<const float4*>(c.mass);
    a.lines = static_cast<const float4*>(c.lines);
    a.out = static_cast<float4*>(c.out);
    a.tension = static_cast<float*>(c.tension);
    a.g = p.g;
    a.dt = c.dt / (float)c.substeps;
    a.nbodies = c.nbodies;
    a.K = c.K;
    HullCall rows = c;  // the hull forces of a substep: the same call, its rows into the handle's buffer
    const dim3 gi((unsigned)(((int64_t)c.nbodies + 255) / 256));
    return run_substeps(
        o, c.nbodies, c.substeps, [&](float4* buf) { rows.out = buf; return hull_launch(o, p, rows, false); },
        [&](const float4* buf, bool last) -> mw_status {
            a.rows = buf;
            a.last = last;
            HIP_TRY(strict_moored_integrate(gi, o->stream, a));
            return MW_OK;
        });
}

// ---- the hull family's entry points ---------------------------------------------------------------------------------------
// One record for hull forces, step bodies and step moored.  Each layer of prepare does its own checks and calls the one below
// (moored_prepare, bodies_prepare, hull_prepare); the host-only checks run triangles first, then body by body the mass row and the slots.
namespace {  // internal linkage, like Stage
struct HullService : HullCall {
    using Plan = HullPlan;
    int64_t count() const { return nbodies; }
    mw_status prepare(mw_ocean* o, int32_t frame, const char* who, HullPlan* p) const {
        return moored ? moored_prepare(o, frame, *this, who, p) : step ? bodies_prepare(o, frame, *this, who, p) : hull_prepare(o, frame, *this, who, p);
    }
    mw_status check_host(const char* who) const {
        if (!triangles_in_range(tris, ntris, nverts)) return fail(MW_EINVAL, who, "triangle index outside [0, nverts)");
        if (!step) return MW_OK;
        for (int32_t b = 0; b < nbodies; b++) {
            const mw_status s = mass_row_check(mass, b, who);
            if (s != MW_OK) return s;
            for (int32_t k = 0; moored && k < K; k++)
                if (!mooring_slot_valid(static_cast<const float*>(lines) + MW_MOORING_NLINE * ((size_t)b * K + k)))
                    return fail(MW_EINVAL, who, "slot " + std::to_string(k) + " of body " + std::to_string(b) +
                                                    " is invalid (a non-finite float, or L0, k or c negative)");
        }
        return MW_OK;
    }
    // mass, lines, out (when stepping) and tension are optional or absent: a NULL array has no region and any alignment
    std::array<Arr, 7> arrays() {
        const size_t nb = (size_t)nbodies, slots = moored ? nb * (size_t)K : 0;
        return {{{&hull, (size_t)nverts * 3 * sizeof(float), IN, 4},
                 {&tris, (size_t)ntris * 3 * sizeof(int32_t), IN, 4},
                 {&bodies, nb * 16 * sizeof(float), step ? INOUT : IN, 16},
                 {&mass, nb * 8 * sizeof(float), IN, 16},
                 {&lines, slots * MW_MOORING_NLINE * sizeof(float), IN, 16},
                 {&out, nb * 8 * sizeof(float), OUT, 16},
                 {&tension, slots * sizeof(float), OUT, 4}}};
    }
    mw_status launch(mw_ocean* o, const HullPlan& p) const {
        return moored ? moored_launch(o, p, *this) : step ? bodies_launch(o, p, *this) : hull_launch(o, p, *this);
    }
};
}  // namespace

mw_status mw_ocean_hull_forces_device(mw_ocean* o, int32_t frame, const void* d_hull_xyz, int32_t nverts, const void* d_triangles,
                                      int32_t ntris, const void* d_bodies, int32_t nbodies, const float* coeffs, int32_t iterations,
                                      void* d_out) {
    const HullService c{{vp(d_hull_xyz), vp(d_triangles), vp(d_bodies), d_out, nverts, ntris, nbodies, iterations, coeffs, false, nullptr, 0.f, 1,
                         false, nullptr, 0, nullptr}};
    return service_device(o, frame, c, "mw_ocean_hull_forces_device",
                          "d_hull_xyz and d_triangles must be 4-byte, d_bodies and d_out 16-byte aligned");
}
mw_status mw_ocean_hull_forces(mw_ocean* o, int32_t frame, const float* hull_xyz, int32_t nverts, const int32_t* triangles, int32_t ntris,
                               const float* bodies, int32_t nbodies, const float* coeffs, int32_t iterations, float* out) {
    const HullService c{{vp(hull_xyz), vp(triangles), vp(bodies), out, nverts, ntris, nbodies, iterations, coeffs, false, nullptr, 0.f, 1, false,
                         nullptr, 0, nullptr}};
    return service_host(o, frame, c, "mw_ocean_hull_forces");
}
mw_status mw_ocean_step_bodies_device(mw_ocean* o, int32_t frame, const void* d_hull_xyz, int32_t nverts, const void* d_triangles,
                                      int32_t ntris, void* d_bodies, const void* d_mass, int32_t nbodies, const float* coeffs,
                                      float dt, int32_t substeps, int32_t iterations, void* d_out) {
    const HullService c{{vp(d_hull_xyz), vp(d_triangles), d_bodies, d_out, nverts, ntris, nbodies, iterations, coeffs, true, vp(d_mass), dt,
                         substeps, false, nullptr, 0, nullptr}};
    return service_device(o, frame, c, "mw_ocean_step_bodies_device",
                          "d_hull_xyz and d_triangles must be 4-byte, d_bodies, d_mass and d_out 16-byte aligned");
}
mw_status mw_ocean_step_bodies(mw_ocean* o, int32_t frame, const float* hull_xyz, int32_t nverts, const int32_t* triangles,
                               int32_t ntris, float* bodies, const float* mass, int32_t nbodies, const float* coeffs, float dt,
                               int32_t substeps, int32_t iterations, float* out) {
    const HullService c{{vp(hull_xyz), vp(triangles), bodies, out, nverts, ntris, nbodies, iterations, coeffs, true, vp(mass), dt, substeps, false,
                         nullptr, 0, nullptr}};
    return service_host(o, frame, c, "mw_ocean_step_bodies");
}
mw_status mw_ocean_step_moored_device(mw_ocean* o, int32_t frame, const void* d_hull_xyz, int32_t nverts, const void* d_triangles,
                                      int32_t ntris, void* d_bodies, const void* d_mass, const void* d_lines, int32_t lines_per_body,
                                      int32_t nbodies, const float* coeffs, float dt, int32_t substeps, int32_t iterations, void* d_out,
                                      void* d_tension) {
    const HullService c{{vp(d_hull_xyz), vp(d_triangles), d_bodies, d_out, nverts, ntris, nbodies, iterations, coeffs, true, vp(d_mass), dt,
                         substeps, true, vp(d_lines), lines_per_body, d_tension}};
    return service_device(o, frame, c, "mw_ocean_step_moored_device",
                          "d_hull_xyz, d_triangles and d_tension must be 4-byte, d_bodies, d_mass, d_lines and d_out 16-byte aligned");
}
mw_status mw_ocean_step_moored(mw_ocean* o, int32_t frame, const float* hull_xyz, int32_t nverts, const int32_t* triangles, int32_t ntris,
                               float* bodies, const float* mass, const float* lines, int32_t lines_per_body, int32_t nbodies,
                               const float* coeffs, float dt, int32_t substeps, int32_t iterations, float* out, float* tension) {
    const HullService c{{vp(hull_xyz), vp(triangles), bodies, out, nverts, ntris, nbodies, iterations, coeffs, true, vp(mass), dt, substeps, true,
                         vp(lines), lines_per_body, tension}};
    return service_host(o, frame, c, "mw_ocean_step_moored");
}

// ---- mixed fleets (csrc/fleet.h) ----------------------------------------------------------------------------------
static_assert(MW_FLEET_MAX_HULLS == MW_FLEET_HULLS && MW_FLEET_NHULL == 5, "fleet.h and the ABI size the hull table alike");
// The arguments of a fleet-forces, step-fleet or step-rigged call; as HullCall, the host and the device form differ only in whose pointers it holds.
// hulls and coeffs are host arrays in both.
struct FleetCall {
    void *hull, *tris, *bodies, *mass, *wrench, *out;
    const int32_t* hulls; const float* coeffs;
    int32_t total_verts, total_tris, nhulls, total_bodies, iterations; float dt; int32_t substeps;
    bool step;  // mw_ocean_step_fleet: mass is required, out is optional, dt and substeps are read
    // rigged (mw_ocean_step_rigged, a stepping call; csrc/rigging.h): lines, the optional targets, K = lines_per_body, the optional tension
    bool rigged; void *lines, *targets; int32_t K; void* tension;
};
// what prepare derives: the mesh of the queried frame, the table of every hull with its coefficients, whether any hull has drag
struct FleetPlan { SqMesh m; FleetTable all; bool drag; };

// Validates a fleet call (the hull table, the sums, the arrays, every hull's coefficients, the stepping arguments) and names the surface
// as hull_prepare does: the velocity query's rules when any hull's row has drag, the surface query's otherwise.
static mw_status fleet_prepare(mw_ocean* o, int32_t frame, const FleetCall& c, const char* who, FleetPlan* p) {
    mw_status s = single_surface_check(o, who);
    if (s != MW_OK) return s;
    if (c.step && !(c.substeps >= 1 && c.substeps <= 64)) return fail(MW_EINVAL, who, "substeps must be in [1, 64]");
    if (c.step && !(c.dt >= 0.f && c.dt <= 3.4e38f)) return fail(MW_EINVAL, who, "dt must be finite and >= 0");
    if (c.nhulls < 1 || c.nhulls > MW_FLEET_MAX_HULLS) return fail(MW_EINVAL, who, "nhulls must be in [1, MW_FLEET_MAX_HULLS]");
    if (!c.hulls || !c.coeffs) return fail(MW_EINVAL, who, "NULL hulls or coeffs");
    if (c.total_bodies < 0 || c.total_verts < 0 || c.total_tris < 0) return fail(MW_EINVAL, who, "total_bodies, total_verts or total_tris < 0");
    const int64_t lim = ((int64_t)1 << 31) - 256;
    int64_t nb = 0, nv = 0, nt = 0;
    for (int h = 0; h < c.nhulls; h++) {
        const int32_t* r = c.hulls + MW_FLEET_NHULL * h;
        const std::string hull = "hull " + std::to_string(h);
        if (r[1] < 3 || r[3] < 1) return fail(MW_EINVAL, who, hull + " needs nverts >= 3 and ntris >= 1");
        if (r[0] < 0 || (int64_t)r[0] + r[1] > c.total_verts) return fail(MW_EINVAL, who, hull + ": its vertex range lies outside hull_xyz");
        if (r[2] < 0 || (int64_t)r[2] + r[3] > c.total_tris) return fail(MW_EINVAL, who, hull + ": its triangle range lies outside triangles");
        if (r[4] < 0) return fail(MW_EINVAL, who, hull + ": nbodies < 0");
        nb += r[4];
        nv += (int64_t)r[4] * r[1];
        nt += (int64_t)r[4] * r[3];
    }
    if (nb != c.total_bodies) return fail(MW_EINVAL, who, "the hulls' nbodies must add up to total_bodies");
    if (nb > lim || nv > lim || nt > lim)
        return fail(MW_EINVAL, who, "total_bodies and the sums of nbodies * nverts and nbodies * ntris must not exceed 2^31 - 256");
    if (c.total_bodies > 0 && (!c.hull || !c.tris || !c.bodies || (c.step ? !c.mass : !c.out))) return fail(MW_EINVAL, who, "NULL array");
    for (int k = 0; k < c.nhulls * MW_HULL_NCOEFFS; k++)
        if (!(c.coeffs[k] >= 0.f && c.coeffs[k] <= 3.4e38f)) return fail(MW_EINVAL, who, "coefficients must be finite and >= 0");
    fleet_table(c.hulls, c.nhulls, ~0u, &p->all);
    p->drag = false;
    for (int h = 0; h < c.nhulls; h++) {
        FleetHull& f = p->all.hull[h];
        hull_coeffs(c.coeffs + MW_HULL_NCOEFFS * h, &f.cf, &f.g, &f.vscale);
        p->drag = p->drag || f.cf.drag;
    }
    const void* mark = c.total_bodies > 0 ? c.bodies : nullptr;
    return p->drag ? query_velocity_prepare(o, frame, MW_QUERY_WORLD, mark, c.total_bodies, c.iterations, mark, who, &p->m)
                   : query_prepare(o, frame, MW_QUERY_WORLD, mark, c.total_bodies, c.iterations, mark, who, &p->m);
}
// Validates a step-rigged call: its own arguments, then the fleet's rules (fleet_prepare).
static mw_status rig_prepare(mw_ocean* o, int32_t frame, const FleetCall& c, const char* who, FleetPlan* p) {
    if (c.K < 1 || c.K > MW_MOORING_MAX_LINES) return fail(MW_EINVAL, who, "lines_per_body must be in [1, MW_MOORING_MAX_LINES]");
    if (c.total_bodies > 0 && !c.lines) return fail(MW_EINVAL, who, "NULL lines");
    return fleet_prepare(o, frame, c, who, p);
}
// the checks only a host form can make: every hull's triangle indices, for stepping every mass and wrench row, and for a rigged call
// every slot and every non-empty slot's target
static mw_status fleet_check_host(const FleetCall& c, const char* who) {
    for (int h = 0; h < c.nhulls; h++) {
        const int32_t* r = c.hulls + MW_FLEET_NHULL * h;
        if (!triangles_in_range(static_cast<const int32_t*>(c.tris) + 3 * (size_t)r[2], r[3], r[1]))
            return fail(MW_EINVAL, who, "hull " + std::to_string(h) + ": triangle index outside [0, nverts)");
    }
    if (!c.step) return MW_OK;
    for (int32_t b = 0; b < c.total_bodies; b++) {
        const mw_status s = mass_row_check(c.mass, b, who);
        if (s != MW_OK) return s;
        if (c.wrench && !fleet_wrench_valid(static_cast<const float*>(c.wrench) + 8 * (size_t)b))
            return fail(MW_EINVAL, who, "the wrench row of body " + std::to_string(b) + " is not finite");
        for (int32_t k = 0; c.rigged && k < c.K; k++) {
            const size_t slot = (size_t)b * c.K + k;
            const float* ln = static_cast<const float*>(c.lines) + MW_MOORING_NLINE * slot;
            const std::string where = "slot " + std::to_string(k) + " of body " + std::to_string(b);
            if (!mooring_slot_valid(ln)) return fail(MW_EINVAL, who, where + " is invalid (a non-finite float, or L0, k or c negative)");
            const int32_t t = c.targets ? static_cast<const int32_t*>(c.targets)[slot] : MW_RIG_ANCHOR;
            if (rig_slot_kind(ln, t, b, c.total_bodies) == MW_RIG_SLOT_BAD)
                return fail(MW_EINVAL, who, where + ": its target " + std::to_string(t) +
                                                " must be MW_RIG_ANCHOR or another body of the call, in [0, total_bodies)");
        }
    }
    return MW_OK;
}

// the table of the hulls in `take`, with the coefficients prepare worked out
static FleetTable fleet_group(const FleetPlan& p, const FleetCall& c, uint32_t take) {
    FleetTable t = p.all;
    fleet_table(c.hulls, c.nhulls, take, &t);
    return t;
}
// k_fleet_vertices, k_fleet_triangles and k_fleet_reduce over a.t (which has bodies), the slab and the partials in the handle's
// hull-forces buffer, the rows into a.rows
static mw_status fleet_rows(mw_ocean* o, FleetArgs& a) {
    HullWork w;
    mw_status s = hull_reserve(o, a.t.total[MW_FLEET_VERTS], a.t.total[MW_FLEET_CHUNKS], a.t.total[MW_FLEET_BODIES], &w);
    if (s != MW_OK) return s;
    a.vslab = w.vslab;
    a.part = w.part;
    if (a.m.period != 0.f) {
        HIP_TRY(tiled_fleet_forces(w.gv, w.gt, w.gr, o->stream, a));
        return MW_OK;
    }
    k_fleet_vertices<<<w.gv, dim3(256), 0, o->stream>>>(a);
    k_fleet_triangles<<<w.gt, dim3(MW_HULL_CHUNK), 0, o->stream>>>(a);
    k_fleet_reduce<<<w.gr, dim3(256), 0, o->stream>>>(a);
    HIP_TRY(hipGetLastError());
    return MW_OK;
}
// The call on the handle's stream (total_bodies > 0): the velocity field once (some hull has drag); forces: the three kernels over
// every hull; stepping: the plan rule of bodies_launch per hull -- the hulls of the one-launch plan in one k_fleet_step launch over all
// their bodies (a periodic handle only), the others through the per-substep launches together.  Bodies do not interact and the surface is frozen, so the two
// groups are independent.
static mw_status fleet_launch(mw_ocean* o, const FleetPlan& p, const FleetCall& c) {
    mw_status s;
    if (p.drag && (s = velocity_to_handle(o)) != MW_OK) return s;
    FleetArgs a{};
    a.m = p.m;
    a.vel = p.drag ? o->vel.vert : nullptr;
    a.iters = sq_iters(c.iterations);
    a.hull = static_cast<const float*>(c.hull); a.tris = static_cast<const int32_t*>(c.tris); a.bodies = static_cast<float4*>(c.bodies);
    a.mass = static_cast<const float4*>(c.mass); a.wrench = static_cast<const float4*>(c.wrench);
    a.out = static_cast<float4*>(c.out);
    if (!c.step) {
        a.t = p.all;
        a.rows = a.out;
        return fleet_rows(o, a);
    }
    a.dt = c.dt / (float)c.substeps;
    a.substeps = c.substeps;
    uint32_t one = 0;
    size_t lds = 0;
    for (int h = 0; h < c.nhulls; h++) {
        const FleetHull& f = p.all.hull[h];
        if (!bodies_one_launch(f.nverts, f.nchunks)) continue;
        one |= 1u << h;
        if (c.hulls[MW_FLEET_NHULL * h + 4] > 0) lds = std::max(lds, bodies_step_lds(f.nverts, f.nchunks));
    }
    // k_fleet_step exists for the tiled surface only (fleet.h, "operand order"): on the one footprint every hull steps per substep,
    // which has the bits of both of mw_ocean_step_bodies' plans
    if (a.m.period == 0.f) one = 0;
    a.t = fleet_group(p, c, one);
    if (a.t.total[MW_FLEET_BODIES] > 0)
        HIP_TRY(tiled_fleet_step(dim3((unsigned)a.t.total[MW_FLEET_BODIES]), lds, MW_BODIES_LDS_MAX, o->stream, a, nullptr, 0, nullptr));
    a.t = fleet_group(p, c, ~one);
    if (a.t.total[MW_FLEET_BODIES] == 0) return MW_OK;
    const dim3 gi((unsigned)(((int64_t)a.t.total[MW_FLEET_BODIES] + 255) / 256));
    return run_substeps(
        o, c.total_bodies, c.substeps, [&](float4* buf) { a.rows = buf; return fleet_rows(o, a); },
        [&](const float4*, bool last) -> mw_status {
            a.last = last;
            if (a.m.period != 0.f) {
                HIP_TRY(tiled_fleet_integrate(gi, o->stream, a));
            } else if (a.wrench) {
                k_fleet_integrate<SqMesh, true><<<gi, dim3(256), 0, o->stream>>>(a);
            } else {
                // the one footprint, no wrench: k_bodies_integrate itself over each hull's bodies -- mw_ocean_step_bodies' bits by
                // construction, where no k_fleet_integrate reproduced them (fleet.h, "operand order")
                for (int h = 0; h < a.t.nhulls; h++) {
                    const FleetHull& f = a.t.hull[h];
                    const int64_t nb = (h + 1 < a.t.nhulls ? a.t.hull[h + 1].first[MW_FLEET_BODIES] : a.t.total[MW_FLEET_BODIES]) - f.first[MW_FLEET_BODIES];
                    if (nb == 0) continue;
                    BodiesArgs ba{};
                    ba.h.nbodies = nb;
                    ba.bodies = a.bodies + 4 * (size_t)f.body_first;
                    ba.mass = a.mass + 2 * (size_t)f.body_first;
                    ba.rows = a.rows + 2 * (size_t)f.body_first;
                    ba.out = a.out ? a.out + 2 * (size_t)f.body_first : nullptr;
                    ba.g = f.g; ba.dt = a.dt; ba.substeps = a.substeps; ba.last = a.last;
                    k_bodies_integrate<<<dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, o->stream>>>(ba);
                }
            }
            HIP_TRY(hipGetLastError());
            return MW_OK;
        });
}

// ---- rigged fleets (csrc/rigging.h) -------------------------------------------------------------------------------
static_assert(MW_RIG_ANCHOR == MW_RIG_TARGET_ANCHOR, "rigging.h and the ABI name the anchor target alike");
// Every substep of a step-rigged call on the handle's stream (total_bodies > 0).  Always the per-substep plan, over every hull of the
// fleet at once: a tow slot reads another body's state at the start of the substep, and a workgroup per body cannot see that without a
// grid-wide barrier.  Per substep fleet_rows on the current state, then k_rigged_integrate, which reads the state from one array and
// writes every body's next state to the other of a pair: the caller's array and the handle's rig buffer.  The first substep reads the
// one that lets the last write land in the caller's array (an odd count starts from a copy in the buffer).
static mw_status rig_launch(mw_ocean* o, const FleetPlan& p, const FleetCall& c) {
    mw_status s;
    if (p.drag && (s = velocity_to_handle(o)) != MW_OK) return s;
    const size_t bytes = (size_t)c.total_bodies * 16 * sizeof(float);
    if ((s = grow_reserve(o, o->rig, bytes, "the step-rigged state buffer")) != MW_OK) return s;
    float4* pair[2] = {static_cast<float4*>(c.bodies), static_cast<float4*>(o->rig.p)};
    int from = c.substeps & 1;
    if (from) HIP_TRY(hipMemcpyAsync(pair[1], pair[0], bytes, hipMemcpyDeviceToDevice, o->stream));
    FleetArgs a{};
    a.m = p.m;
    a.vel = p.drag ? o->vel.vert : nullptr;
    a.iters = sq_iters(c.iterations);
    a.hull = static_cast<const float*>(c.hull); a.tris = static_cast<const int32_t*>(c.tris);
    a.t = p.all;
    RigArgs r{};
    r.mass = static_cast<const float4*>(c.mass); r.wrench = static_cast<const float4*>(c.wrench);
    r.lines = static_cast<const float4*>(c.lines); r.targets = static_cast<const int32_t*>(c.targets);
    r.out = static_cast<float4*>(c.out); r.tension = static_cast<float*>(c.tension);
    r.dt = c.dt / (float)c.substeps;
    r.K = c.K;
    r.t = p.all;
    const dim3 gi((unsigned)(((int64_t)c.total_bodies + 255) / 256));
    return run_substeps(
        o, c.total_bodies, c.substeps, [&](float4* buf) { a.bodies = pair[from]; a.rows = buf; return fleet_rows(o, a); },
        [&](const float4* buf, bool last) -> mw_status {
            r.snap = pair[from]; r.next = pair[from ^ 1]; r.rows = buf; r.last = last;
            from ^= 1;
            HIP_TRY(strict_rigged_integrate(gi, o->stream, r));
            return MW_OK;
        });
}

namespace {  // internal linkage, like Stage
struct FleetService : FleetCall {
    using Plan = FleetPlan;
    int64_t count() const { return total_bodies; }
    mw_status prepare(mw_ocean* o, int32_t frame, const char* who, FleetPlan* p) const {
        return rigged ? rig_prepare(o, frame, *this, who, p) : fleet_prepare(o, frame, *this, who, p);
    }
    mw_status check_host(const char* who) const { return fleet_check_host(*this, who); }
    // mass (forces), wrench, when stepping out, and a rigged call's targets and tension are optional or absent
    std::array<Arr, 9> arrays() {
        const size_t nb = (size_t)total_bodies, slots = rigged ? nb * (size_t)K : 0;
        return {{{&hull, (size_t)total_verts * 3 * sizeof(float), IN, 4},
                 {&tris, (size_t)total_tris * 3 * sizeof(int32_t), IN, 4},
                 {&bodies, nb * 16 * sizeof(float), step ? INOUT : IN, 16},
                 {&mass, nb * 8 * sizeof(float), IN, 16},
                 {&wrench, nb * 8 * sizeof(float), IN, 16},
                 {&lines, slots * MW_MOORING_NLINE * sizeof(float), IN, 16},
                 {&targets, slots * sizeof(int32_t), IN, 4},
                 {&out, nb * 8 * sizeof(float), OUT, 16},
                 {&tension, slots * sizeof(float), OUT, 4}}};
    }
    mw_status launch(mw_ocean* o, const FleetPlan& p) const { return rigged ? rig_launch(o, p, *this) : fleet_launch(o, p, *this); }
};
}  // namespace
// Fleets do not read the column yet: with draught on (mw_ocean_set_draught) every fleet entry point refuses, before any other work --
// its alignment test included -- and after nothing but the NULL handle, which the service reports.
static mw_status fleet_entry(mw_ocean* o, int32_t frame, const FleetService& c, const char* who, bool device) {
    if (o) HIP_TRY(hipSetDevice(o->device));
    if (o && o->draught)
        return fail(MW_ESTATE, who, "fleets do not read the water column yet: the handle has draught on (mw_ocean_set_draught(o, 0) first, or "
                                    "mw_ocean_hull_forces / mw_ocean_step_bodies per hull)");
    if (!device) return service_host(o, frame, c, who);
    return service_device(o, frame, c, who,
                          c.rigged ? "d_hull_xyz, d_triangles, d_targets and d_tension must be 4-byte, d_bodies, d_mass, d_wrench, d_lines and "
                                     "d_out 16-byte aligned"
                                   : "d_hull_xyz and d_triangles must be 4-byte, d_bodies, d_mass, d_wrench and d_out 16-byte aligned");
}

mw_status mw_ocean_fleet_forces(mw_ocean* o, int32_t frame, const float* hull_xyz, int32_t total_verts, const int32_t* triangles,
                                int32_t total_tris, const int32_t* hulls, int32_t nhulls, const float* bodies, int32_t total_bodies,
                                const float* coeffs, int32_t iterations, float* out) {
    const FleetService c{{vp(hull_xyz), vp(triangles), vp(bodies), nullptr, nullptr, out, hulls, coeffs, total_verts, total_tris, nhulls,
                          total_bodies, iterations, 0.f, 1, false, false, nullptr, nullptr, 0, nullptr}};
    return fleet_entry(o, frame, c, "mw_ocean_fleet_forces", false);
}
mw_status mw_ocean_fleet_forces_device(mw_ocean* o, int32_t frame, const void* d_hull_xyz, int32_t total_verts, const void* d_triangles,
                                       int32_t total_tris, const int32_t* hulls, int32_t nhulls, const void* d_bodies,
                                       int32_t total_bodies, const float* coeffs, int32_t iterations, void* d_out) {
    const FleetService c{{vp(d_hull_xyz), vp(d_triangles), vp(d_bodies), nullptr, nullptr, d_out, hulls, coeffs, total_verts, total_tris, nhulls,
                          total_bodies, iterations, 0.f, 1, false, false, nullptr, nullptr, 0, nullptr}};
    return fleet_entry(o, frame, c, "mw_ocean_fleet_forces_device", true);
}
mw_status mw_ocean_step_fleet(mw_ocean* o, int32_t frame, const float* hull_xyz, int32_t total_verts, const int32_t* triangles,
                              int32_t total_tris, const int32_t* hulls, int32_t nhulls, float* bodies, const float* mass, const float* wrench,
                              int32_t total_bodies, const float* coeffs, float dt, int32_t substeps, int32_t iterations, float* out) {
    const FleetService c{{vp(hull_xyz), vp(triangles), bodies, vp(mass), vp(wrench), out, hulls, coeffs, total_verts, total_tris, nhulls,
                          total_bodies, iterations, dt, substeps, true, false, nullptr, nullptr, 0, nullptr}};
    return fleet_entry(o, frame, c, "mw_ocean_step_fleet", false);
}
mw_status mw_ocean_step_fleet_device(mw_ocean* o, int32_t frame, const void* d_hull_xyz, int32_t total_verts, const void* d_triangles,
                                     int32_t total_tris, const int32_t* hulls, int32_t nhulls, void* d_bodies, const void* d_mass,
                                     const void* d_wrench, int32_t total_bodies, const float* coeffs, float dt, int32_t substeps,
                                     int32_t iterations, void* d_out) {
    const FleetService c{{vp(d_hull_xyz), vp(d_triangles), d_bodies, vp(d_mass), vp(d_wrench), d_out, hulls, coeffs, total_verts, total_tris,
                          nhulls, total_bodies, iterations, dt, substeps, true, false, nullptr, nullptr, 0, nullptr}};
    return fleet_entry(o, frame, c, "mw_ocean_step_fleet_device", true);
}

mw_status mw_ocean_step_rigged(mw_ocean* o, int32_t frame, const float* hull_xyz, int32_t total_verts, const int32_t* triangles,
                               int32_t total_tris, const int32_t* hulls, int32_t nhulls, float* bodies, const float* mass, const float* wrench,
                               const float* lines, const int32_t* targets, int32_t lines_per_body, int32_t total_bodies,
                               const float* coeffs, float dt, int32_t substeps, int32_t iterations, float* out, float* tension) {
    const FleetService c{{vp(hull_xyz), vp(triangles), bodies, vp(mass), vp(wrench), out, hulls, coeffs, total_verts, total_tris, nhulls,
                          total_bodies, iterations, dt, substeps, true, true, vp(lines), vp(targets), lines_per_body, tension}};
    return fleet_entry(o, frame, c, "mw_ocean_step_rigged", false);
}
mw_status mw_ocean_step_rigged_device(mw_ocean* o, int32_t frame, const void* d_hull_xyz, int32_t total_verts, const void* d_triangles,
                                      int32_t total_tris, const int32_t* hulls, int32_t nhulls, void* d_bodies, const void* d_mass,
                                      const void* d_wrench, const void* d_lines, const void* d_targets, int32_t lines_per_body,
                                      int32_t total_bodies, const float* coeffs, float dt, int32_t substeps, int32_t iterations,
                                      void* d_out, void* d_tension) {
    const FleetService c{{vp(d_hull_xyz), vp(d_triangles), d_bodies, vp(d_mass), vp(d_wrench), d_out, hulls, coeffs, total_verts, total_tris,
                          nhulls, total_bodies, iterations, dt, substeps, true, true, vp(d_lines), vp(d_targets), lines_per_body, d_tension}};
    return fleet_entry(o, frame, c, "mw_ocean_step_rigged_device", true);
}

// ---- raycasts (csrc/raycast.h) -------------------------------------------------------------------------------------
// The surface query's validation and mesh (query_prepare, world mode), then the hierarchy of that mesh into the handle's tree buffer
// (k_rc_build_leaves, and k_rc_build_top for trees deeper than 4 levels) and one lane per ray (k_raycast), all on the handle's stream.
// A periodic handle is refused: this cast reads the one footprint.  The tiled surface has its own entry point, mw_ocean_raycast_tiled.
static mw_status raycast_prepare(mw_ocean* o, int32_t frame, const void* rays, int64_t n, const void* out, const char* who, SqMesh* m) {
    mw_status s = query_prepare(o, frame, MW_QUERY_WORLD, rays, n, 0, out, who, m);
    if (s == MW_OK && m->period != 0.f)
        return fail(MW_ESTATE, who, "raycasts do not tile yet: the handle is periodic (mw_ocean_set_periodic(o, 0) first, or mw_ocean_raycast_tiled "
                                    "for the tiled surface)");
    return s;
}
extern "C++" {
// The hierarchy of a surface of side x side grid lines into the handle's tree buffer, on the handle's stream: leaves(grid, tree) launches
// the leaf builder of the surface, k_rc_build_top the levels above for trees deeper than 4.  *tr names the tree, its boxes included.
template <class Leaves>
static mw_status raycast_tree(mw_ocean* o, int side, Leaves leaves, RcTree* tr) {
    int B = sw(SW_RC_BLOCK);
    if (B <= 0) B = MW_RC_DEFAULT_BLOCK;
    const int minB = (side - 2) / (1 << MW_RC_MAX_LEVEL) + 1;  // at most 2^MW_RC_MAX_LEVEL leaves per side
    *tr = rc_tree(nullptr, side, B < minB ? minB : B);
    mw_status s = grow_reserve(o, o->rc_tree, (size_t)rc_nodes(tr->D) * 8 * sizeof(float), "the raycast hierarchy");
    if (s != MW_OK) return s;
    tr->box = static_cast<float*>(o->rc_tree.p);
    const int T = tr->D >= 4 ? 16 : (1 << tr->D), tiles = (1 << tr->D) / T;
    HIP_TRY(leaves(dim3((unsigned)(tiles * tiles)), *tr));
    if (tr->D > 4) k_rc_build_top<<<dim3(1), dim3(256), 0, o->stream>>>(*tr);
    HIP_TRY(hipGetLastError());
    return MW_OK;
}
}  // extern "C++"
// the footprint's tree: what mw_ocean_raycast casts through and mw_debug_raycast_tree returns
static mw_status raycast_build(mw_ocean* o, const SqMesh& m, RcTree* tr) {
    return raycast_tree(o, m.R, [&](dim3 grid, const RcTree& t) {
        k_rc_build_leaves<SqMesh><<<grid, dim3(256), 0, o->stream>>>(m, t);
        return hipSuccess;
    }, tr);
}
namespace {
struct Raycast : PointCall {
    mw_status prepare(mw_ocean* o, int32_t frame, const char* who, SqMesh* m) const { return raycast_prepare(o, frame, pts, n, out, who, m); }
    std::array<Arr, 3> arrays() { return {{{&pts, floats(8), IN, 16}, {&out, floats(8), OUT, 16}, {&hit, floats(2), OUT, 8}}}; }  // hit: optional
    mw_status launch(mw_ocean* o, const SqMesh& m) const {
        RcTree tr;
        mw_status s = raycast_build(o, m, &tr);
        if (s != MW_OK) return s;
        k_raycast<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, o->stream>>>(m, tr, static_cast<const float4*>(pts), n, static_cast<float4*>(out),
                                                                                  static_cast<int2*>(hit));
        HIP_TRY(hipGetLastError());
        return MW_OK;
    }
};
}  // namespace

mw_status mw_ocean_raycast_device(mw_ocean* o, int32_t frame, const void* d_rays, int64_t n, void* d_out, void* d_hit) {
    return service_device(o, frame, Raycast{{vp(d_rays), d_out, d_hit, n, MW_QUERY_WORLD, 0, 0}}, "mw_ocean_raycast_device",
                          "d_rays and d_out must be 16-byte and d_hit 8-byte aligned");
}
mw_status mw_ocean_raycast(mw_ocean* o, int32_t frame, const float* rays, int64_t n, float* out, int32_t* hit) {
    return service_host(o, frame, Raycast{{vp(rays), out, hit, n, MW_QUERY_WORLD, 0, 0}}, "mw_ocean_raycast");
}

// ---- tiled raycasts (csrc/raycast_tiled.h) ------------------------------------------------------------------------------
// The entry point names its surface: the handle's periodic switch is neither read nor changed.  Handle rules first (batched, OceanRenderer,
// a grid that does not repeat), then the arguments and the frame (query_prepare), and the mesh carries the grid's period whatever the switch
// says.  The hierarchy of one tile goes into the same tree buffer as mw_ocean_raycast's (k_rc_build_leaves<SqTiled> in surface_tiled.hip, then
// k_rc_build_top for trees deeper than 4 levels), then one lane per ray (k_raycast_tiled), all on the handle's stream.
static mw_status raycast_tiled_prepare(mw_ocean* o, int32_t frame, const void* rays, int64_t n, int32_t reach, const void* out, const char* who,
                                       SqMesh* m) {
    mw_status s = single_surface_check(o, who);
    if (s != MW_OK) return s;
    if (o->sem != MW_SEM_FFTMESH) return fail(MW_ESTATE, who, "an OceanRenderer mesh does not tile (mw_ocean_set_periodic)");
    if (reach < 0 || reach > MW_RC_MAX_REACH) return fail(MW_EINVAL, who, "reach must be in [0, MW_RC_MAX_REACH]");
    const float P = grid_period(o);
    if (P == 0.f)
        return fail(MW_ENOTCOMMENSURATE, who, "the frame repeats only where unit_width * resolution == length and the resolution is even");
    s = query_prepare(o, frame, MW_QUERY_WORLD, rays, n, 0, out, who, m);
    m->period = P;
    return s;
}
// the tree of one tile (rct_tree: its N x N cells, grid line N the wrapped line 0): what mw_ocean_raycast_tiled casts through and
// mw_debug_raycast_tree returns
static mw_status raycast_tiled_build(mw_ocean* o, const SqMesh& m, RcTree* tr) {
    return raycast_tree(o, m.R + 1, [&](dim3 grid, const RcTree& t) { return tiled_raycast_build_leaves(grid, o->stream, m, t); }, tr);
}
namespace {
struct RaycastTiled : PointCall {
    mw_status prepare(mw_ocean* o, int32_t frame, const char* who, SqMesh* m) const {
        return raycast_tiled_prepare(o, frame, pts, n, reach, out, who, m);
    }
    std::array<Arr, 3> arrays() { return {{{&pts, floats(8), IN, 16}, {&out, floats(8), OUT, 16}, {&hit, floats(4), OUT, 16}}}; }  // hit: optional
    mw_status launch(mw_ocean* o, const SqMesh& m) const {
        RcTree tr;
        mw_status s = raycast_tiled_build(o, m, &tr);
        if (s != MW_OK) return s;
        HIP_TRY(tiled_raycast(dim3((unsigned)((n + 255) / 256)), o->stream, m, tr, static_cast<const float4*>(pts), n, reach,
                              static_cast<float4*>(out), static_cast<int4*>(hit)));
        return MW_OK;
    }
};
}  // namespace

mw_status mw_ocean_raycast_tiled_device(mw_ocean* o, int32_t frame, const void* d_rays, int64_t n, int32_t reach, void* d_out, void* d_hit) {
    return service_device(o, frame, RaycastTiled{{vp(d_rays), d_out, d_hit, n, MW_QUERY_WORLD, 0, reach}}, "mw_ocean_raycast_tiled_device",
                          "d_rays, d_out and d_hit must be 16-byte aligned");
}
mw_status mw_ocean_raycast_tiled(mw_ocean* o, int32_t frame, const float* rays, int64_t n, int32_t reach, float* out, int32_t* hit) {
    return service_host(o, frame, RaycastTiled{{vp(rays), out, hit, n, MW_QUERY_WORLD, 0, reach}}, "mw_ocean_raycast_tiled");
}

// ---- the water column (csrc/water_column.h) -----------------------------------------------------------------------------
// FFTMesh handles only: an OceanRenderer mesh samples clamp-addressed textures (DESIGN.md section 7g) and has no column.
static mw_status column_handle_check(mw_ocean* o, const char* who) {
    if (!o) return fail(MW_EINVAL, who, "NULL handle");
    if (o->sem != MW_SEM_FFTMESH)
        return fail(MW_EINVAL, who, "an OceanRenderer or batched handle has no column (its mesh samples clamp-addressed textures): FFTMesh handles only");
    return MW_OK;
}

mw_status mw_ocean_set_column(mw_ocean* o, const float* depths, int32_t nlayers) {
    const char* who = "mw_ocean_set_column";
    mw_status s = column_handle_check(o, who);
    if (s != MW_OK) return s;
    if (nlayers != 0 && (nlayers < 2 || nlayers > MW_COLUMN_MAX_LAYERS)) return fail(MW_EINVAL, who, "nlayers must be 0 or in [2, MW_COLUMN_MAX_LAYERS]");
    if (nlayers > 0) {
        if (!depths) return fail(MW_EINVAL, who, "NULL depths");
        if (depths[0] != 0.f) return fail(MW_EINVAL, who, "depths[0] must be 0 (layer 0 is the surface)");
        for (int l = 1; l < nlayers; l++)
            if (!(depths[l] > depths[l - 1] && depths[l] <= 3.4e38f)) return fail(MW_EINVAL, who, "depths must be finite and strictly increasing");
    }
    HIP_TRY(hipSetDevice(o->device));
    HIP_TRY(hipStreamSynchronize(o->stream));  // work on the stream may still read the old layers
    col_release(o->col);
    o->col.L = nlayers;
    for (int l = 0; l < MW_COL_MAX_LAYERS; l++) o->col.depth[l] = l < nlayers ? depths[l] : 0.f;
    return MW_OK;
}

mw_status mw_ocean_get_column(mw_ocean* o, float* depths, int32_t* nlayers) {
    mw_status s = column_handle_check(o, "mw_ocean_get_column");
    if (s != MW_OK) return s;
    if (nlayers) *nlayers = o->col.L;
    if (depths) for (int l = 0; l < o->col.L; l++) depths[l] = o->col.depth[l];
    return MW_OK;
}

// Draught: a switch on the handle, read per call by the hull family (hull_prepare, hull_launch, bodies_launch) and refused by the fleets.
// Only a handle that can have a column takes it; no column has to be set yet.
mw_status mw_ocean_set_draught(mw_ocean* o, int32_t on) {
    const char* who = "mw_ocean_set_draught";
    if (!o) return fail(MW_EINVAL, who, "NULL handle");
    if (on != 0 && on != 1) return fail(MW_EINVAL, who, "on must be 0 or 1");
    mw_status s = column_handle_check(o, who);
    if (s != MW_OK) return s;
    o->draught = on != 0;
    return MW_OK;
}
mw_status mw_ocean_get_draught(mw_ocean* o, int32_t* on) {
    if (!o) return fail(MW_EINVAL, "mw_ocean_get_draught", "NULL handle");
    if (on) *on = o->draught ? 1 : 0;
    return MW_OK;
}

// Validates a column call: the handle, then the surface query's argument and frame rules (query_prepare), then the state -- a column, and
// a frame that is still the spectrum's (the frame_behind rule of mw_ocean_query_velocity).  Names the surface mesh, period included.
static mw_status column_prepare(mw_ocean* o, int32_t frame, int32_t mode, const void* xyz, int64_t n, int32_t iterations, const void* out,
                                const char* who, SqMesh* m) {
    mw_status s = column_handle_check(o, who);
    if (s == MW_OK) s = query_prepare(o, frame, mode, xyz, n, iterations, out, who, m);
    if (s != MW_OK) return s;
    if (o->col.L == 0) return fail(MW_ESTATE, who, "no column set (mw_ocean_set_column first)");
    if (o->frame_behind)
        return fail(MW_ESTATE, who, "the spectrum or phase changed after the latest frame: the surface and the layers would belong to "
                                    "different instants (make a frame first)");
    return MW_OK;
}
// The layers of the latest frame, on the handle's stream: buffers on first use, the weighted spectra once per spectrum and column (one
// k_column_weight per layer and, on the FFT path, two k_prep), the layer arrays once per frame -- per layer the frame passes on the
// attenuated spectrum and the velocity passes on its weighted twin, exactly as velocity_run runs them.  Layer 0's velocity (vel.vert)
// is made current here too.  Writes only the column's buffers, the handle's velocity buffers and the frame pipeline's work space.
static mw_status column_build(mw_ocean* o) {
    ColState& c = o->col;
    const int N = o->N;
    const size_t NN = (size_t)N * N;
    mw_status s = MW_OK;
    if (!c.white) {  // the last buffer allocated: a failure half-way frees them all, and the next call starts again
        for (int l = 1; l < c.L && s == MW_OK; l++) {
            ColLayer& y = c.layer[l];
            if ((s = fm_spectrum_alloc(y.psp, N, o->use_fft)) != MW_OK || (s = fm_spectrum_alloc(y.vsp, N, o->use_fft)) != MW_OK ||
                (s = dmalloc(&y.pos, 3 * NN)) != MW_OK)
                break;
            s = dmalloc(&y.vel, 3 * NN);
        }
        if (s != MW_OK || (s = dmalloc(&c.norm, 3 * NN)) != MW_OK || (s = dmalloc(&c.white, NN)) != MW_OK) {
            col_release(c);
            return s;
        }
    }
    if (!c.ready) {
        for (int l = 1; l < c.L; l++) {
            ColLayer& y = c.layer[l];
            HIP_TRY(column_weight_launch(o->stream, N, o->p.length, o->p.gravity, c.depth[l], o->fm.sp.h0, o->fm.sp.h0c, y.psp.h0, y.psp.h0c, y.vsp.h0,
                                         y.vsp.h0c));
            if (o->use_fft && ((s = fm_prep(y.psp, N, o->p.length, o->p.gravity, o->fm.Wpre, o->stream)) != MW_OK ||
                               (s = fm_prep(y.vsp, N, o->p.length, o->p.gravity, o->fm.Wpre, o->stream)) != MW_OK))
                return s;
        }
        column_spectra_built(o);
    }
    if (c.built && o->vel.vert) return MW_OK;
    if ((s = velocity_to_handle(o)) != MW_OK) return s;
    OceanConsts C = consts_of(o);
    C.choppiness = o->fm.s_chop;  // the frame's choppiness, as velocity_run
    const unsigned nb = (unsigned)((NN + 255) / 256);
    for (int l = 1; l < c.L; l++) {
        ColLayer& y = c.layer[l];
        if (!o->use_fft) {
            if ((s = direct_evaluate(o->direct, C, y.psp.h0, y.psp.h0c, o->fm.s_t, y.pos, c.norm, c.white, 1, o->stream)) != MW_OK) return s;
            if ((s = direct_evaluate(o->direct, C, y.vsp.h0, y.vsp.h0c, o->fm.s_t, y.vel, c.norm, c.white, 1, o->stream)) != MW_OK) return s;
            hipLaunchKernelGGL(k_velocity_from_hds, dim3(nb), dim3(256), 0, o->stream, N, C.choppiness, o->direct.hds, y.vel);
            HIP_TRY(hipGetLastError());
            continue;
        }
        if ((s = fm_evaluate(o->fm, y.psp, C, &o->fm.s_t, 1, y.pos, c.norm, c.white, 1, o->stream)) != MW_OK) return s;
        if ((s = fm_evaluate(o->fm, y.vsp, C, &o->fm.s_t, 1, y.vel, c.norm, c.white, 1, o->stream, true)) != MW_OK) return s;
    }
    column_layers_built(o);
    return MW_OK;
}
static ColTable column_table(const mw_ocean* o, const SqMesh& m) {
    ColTable tb{};
    tb.L = o->col.L;
    for (int l = 0; l < tb.L; l++) {
        tb.depth[l] = o->col.depth[l];
        tb.pos[l] = l ? o->col.layer[l].pos : m.vert;
        tb.vel[l] = l ? o->col.layer[l].vel : o->vel.vert;
    }
    return tb;
}
namespace {
struct QueryColumn : PointCall {
    mw_status prepare(mw_ocean* o, int32_t frame, const char* who, SqMesh* m) const {
        return column_prepare(o, frame, mode, pts, n, iterations, out, who, m);
    }
    std::array<Arr, 2> arrays() { return {{{&pts, floats(4), IN, 16}, {&out, floats(MW_COL_NOUT), OUT, 16}}}; }
    mw_status launch(mw_ocean* o, const SqMesh& m) const {
        mw_status s = column_build(o);
        if (s != MW_OK) return s;
        HIP_TRY(column_query_launch(o->stream, m, column_table(o, m), mode, sq_iters(iterations), static_cast<const float4*>(pts), n,
                                    static_cast<float4*>(out)));
        return MW_OK;
    }
};
}  // namespace

mw_status mw_ocean_column_layers(mw_ocean* o, int32_t frame, int32_t layer, void** d_positions, void** d_velocities) {
    const char* who = "mw_ocean_column_layers";
    if (o) HIP_TRY(hipSetDevice(o->device));
    SqMesh m{};
    mw_status s = column_handle_check(o, who);
    if (s != MW_OK) return s;
    if (layer < 0 || layer >= MW_COLUMN_MAX_LAYERS || (o->col.L > 0 && layer >= o->col.L)) return fail(MW_EINVAL, who, "layer out of range");
    if ((s = column_prepare(o, frame, MW_QUERY_WORLD, nullptr, 0, 0, nullptr, who, &m)) != MW_OK || (s = column_build(o)) != MW_OK) return s;
    const ColTable tb = column_table(o, m);
    if (d_positions) *d_positions = const_cast<float*>(tb.pos[layer]);
    if (d_velocities) *d_velocities = const_cast<float*>(tb.vel[layer]);
    return MW_OK;
}

mw_status mw_ocean_query_column_device(mw_ocean* o, int32_t frame, int32_t mode, const void* d_xyz_, int64_t n, int32_t iterations, void* d_out) {
    return service_device(o, frame, QueryColumn{{vp(d_xyz_), d_out, nullptr, n, mode, iterations, 0}}, "mw_ocean_query_column_device",
                          "d_xyz_ and d_out must be 16-byte aligned");
}
mw_status mw_ocean_query_column(mw_ocean* o, int32_t frame, int32_t mode, const float* xyz_, int64_t n, int32_t iterations, float* out) {
    return service_host(o, frame, QueryColumn{{vp(xyz_), out, nullptr, n, mode, iterations, 0}}, "mw_ocean_query_column");
}
