// debug_hooks.inc -- the hooks of include/mistral_water_hooks.h (included by mistral_water.hip inside extern "C", where their kernels stand in
// the code object): the profiling hook, then mw_debug_* with the k_dbg_* kernels (k_dbg_stream, a template, stands ahead of extern "C").

// per-launch durations -> (mean, median, p10, p90, min, max), milliseconds
static void launch_stats(std::vector<float>& v, float* out6) {
    std::sort(v.begin(), v.end());
    const size_t n = v.size();
    double acc = 0.0;
    for (float x : v) acc += x;
    auto pct = [&](double q) { return v[(size_t)std::min<double>((double)n - 1.0, std::floor(q * (double)(n - 1) + 0.5))]; };
    out6[0] = (float)(acc / (double)n); out6[1] = pct(0.5); out6[2] = pct(0.1); out6[3] = pct(0.9); out6[4] = v.front(); out6[5] = v.back();
}
// ---- the profiling hook: the launches of one call of the handle's path, timed in situ with a HIP event between every two.  profile_or /
// profile_direct / profile_fft say what one timed call of their path is; KernelTimes owns the samples and everything reported from them.
namespace {  // internal linkage, like Stage
struct KernelTimes {
    int n = 0;  // kernels of the profiled path, and their names
    const char* const* names = nullptr;
    bool report_failed = false;  // the FFT path reports its names (and zero means) even when a launch failed
    std::vector<float> per[4];   // per kernel: one duration per timed call, in call order
    void add(const float* ms) { for (int k = 0; k < n; k++) per[k].push_back(ms[k]); }
    // the mean is the sum in call order (taken before launch_stats sorts); stats only for a run whose launches all succeeded
    void report(int iters, bool ok, float* ms_out, float* stats_out, const char** names_out, int32_t* nkernels) {
        for (int k = 0; k < n; k++) {
            double acc = 0.0;
            for (float x : per[k]) acc += x;
            ms_out[k] = (float)(acc / iters);
            if (names_out) names_out[k] = names[k];
            if (stats_out && ok) launch_stats(per[k], stats_out + 6 * k);
        }
        *nkernels = n;
    }
};
struct Events : std::vector<hipEvent_t> {  // n HIP events, created here and destroyed with the scope
    explicit Events(size_t n) : std::vector<hipEvent_t>(n) { for (auto& e : *this) hipEventCreate(&e); }
    ~Events() { for (auto& e : *this) hipEventDestroy(e); }
};
}  // namespace
// warm-up: the first ~10 ms after idle run at reduced clocks (bench.py preheats its timed region for the same reason): 120 ms of `call`
static mw_status warm_up(hipStream_t st, const std::function<mw_status()>& call) {
    mw_status s = MW_OK;
    const auto t0 = std::chrono::steady_clock::now();
    do {
        for (int w = 0; w < 2 && s == MW_OK; w++) s = call();
        hipStreamSynchronize(st);
    } while (s == MW_OK && std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() < 0.12);
    return s;
}
// OceanRenderer: nsteps frames per enqueue (1: the lone-frame plan); the launches of a call follow one another as in
// mw_ocean_generate_texture[_steps]_device; the frames stay in the handle.  The phase ADVANCES.
static mw_status profile_or(mw_ocean* o, int nsteps, int iters, KernelTimes& kt) {
    if (nsteps > 1 && o->orr.tiles != 1) return fail(MW_ESTATE, "mw_ocean_profile_kernels: a batched handle advances one frame per call");
    static const char* rnames[4] = {"k_or_pass1 (dispersion + spectrum + transform along py)", "k_or_pass2 (transform along px, height / displacement)",
                                    "k_or_normal_white", "copies (k_or_copy_frame: the last frame becomes the handle's latest)"};
    static const char* snames[4] = {"k_or_pass1_steps (phase chain + spectra + transform along py, all frames)", rnames[1], rnames[2], rnames[3]};
    kt.n = 4; kt.names = nsteps == 1 ? rnames : snames;
    float dts[MW_OR_MAX_FRAMES];
    for (int k = 0; k < MW_OR_MAX_FRAMES; k++) dts[k] = 1.0f / 60.0f;
    frame_or_lone(o);
    auto call = [&](hipEvent_t* ev) { return or_frames(o->orr, o->p.choppiness, dts, nsteps, false, {nullptr, nullptr, nullptr, nullptr}, o->stream, ev); };
    mw_status s = warm_up(o->stream, [&] { return call(nullptr); });
    if (s != MW_OK) return s;
    // events of one call, per chunk j of frames (one chunk in the lone-frame plan): [3j] before its spectrum launch, [3j + 1] after it,
    // [3j + 2] after its pass 2, [3j + 3] after its normal / whitecap pass; [3 nch + 1] after the copies.  All calls first, one wait.
    const int nch = nsteps == 1 ? 1 : or_steps_chunks(o->orr.M, nsteps);
    const size_t per_it = 2 + 3 * (size_t)nch;
    Events ev(per_it * (size_t)iters);
    for (int it = 0; it < iters && s == MW_OK; it++) s = call(&ev[per_it * (size_t)it]);
    hipStreamSynchronize(o->stream);
    for (int it = 0; it < iters && s == MW_OK; it++) {
        hipEvent_t* e = &ev[per_it * (size_t)it];
        float m[4] = {0.f, 0.f, 0.f, 0.f}, x = 0.f;
        for (int j = 0; j < nch; j++)
            for (int k = 0; k < 3; k++) { hipEventElapsedTime(&x, e[3 * j + k], e[3 * j + k + 1]); m[k] += x; }
        hipEventElapsedTime(&m[3], e[3 * nch], e[3 * nch + 1]);
        kt.add(m);
    }
    if (s != MW_OK) return s;
    const bool kept[4] = {true, true, true, true};
    frame_or_steps(o, nsteps, kept, -1);  // the hook has always left the steps tail unset: mw_ocean_velocity takes frame -1 only after it
    return MW_OK;
}
// FFTMesh direct-sum path: kernel 0 = the four GEMM launches of one step, kernel 1 = spectrum + assembly + whitecap.  Five calls warm up;
// every timed call is waited for on its own.
static mw_status profile_direct(mw_ocean* o, int nsteps, int iters, KernelTimes& kt) {
    if (nsteps != 1) return fail(MW_EINVAL, "mw_ocean_profile_kernels: the direct-sum path evaluates one step per enqueue");
    static const char* gnames[2] = {"k_gemm_f32_mfma (4 launches: z sum, x sum)", "k_direct_spec + k_direct_assemble + k_direct_white"};
    static const char* znames[2] = {"k_czt (2 launches: spectrum + chirp-z along j, chirp-z along i)", "k_czt_assemble_white"};
    static const char* fnames[2] = {"k_czt (spectrum + chirp-z along j)", "k_czt_rows_assemble (chirp-z along i + vertices, normals, whitecap: one launch)"};
    static const char* onames[2] = {"(no separate launch)", "k_czt_one (both axes + vertices, normals, whitecap: one workgroup, one launch)"};
    kt.n = 2; kt.names = gnames;
    if (o->direct.use_czt) {  // the names follow the plan czt_evaluate runs (czt_plan: the one place that decides)
        const CztPlan plan = czt_plan(o->direct, o->N);
        kt.names = plan == CZT_PLAN_ONE ? onames : (plan == CZT_PLAN_TWO ? fnames : znames);
    }
    FmState& f = o->fm;
    auto call = [&](float t, hipEvent_t* ev) {
        return direct_evaluate(o->direct, consts_of(o), f.sp.h0, f.sp.h0c, t, f.s_vert, f.s_norm, f.s_white, 1, o->stream, ev);
    };
    Events ev(4);
    frame_fftmesh_overwritten(o);  // by the launches below (whitecap scalar, stride 1)
    mw_status s = MW_OK;
    for (int w = 0; w < 5 && s == MW_OK; w++) s = call(1.0f, nullptr);
    for (int it = 0; it < iters && s == MW_OK; it++) {
        s = call(1.0f + (float)it / 60.f, &ev[0]);
        hipEventRecord(ev[3], o->stream);
        hipEventSynchronize(ev[3]);
        float d[3] = {0.f, 0.f, 0.f};
        for (int k = 0; k < 3; k++) hipEventElapsedTime(&d[k], ev[k], ev[k + 1]);
        const float m[2] = {d[1], d[0] + d[2]};
        kt.add(m);
    }
    if (s != MW_OK) return s;
    frame_fftmesh_made(o, 1.0f + (float)(iters - 1) / 60.f, 1);  // the chirp-z / direct kernels above wrote the host-API frame
    return MW_OK;
}
// FFTMesh FFT path: the two kernels alternate exactly as in mw_ocean_evaluate_device (pass 2 of a batch follows its pass 1), through
// fm_evaluate with its event between the passes.  All calls first, one wait.
static mw_status profile_fft(mw_ocean* o, int nsteps, int iters, KernelTimes& kt) {
    FmState& f = o->fm;
    const size_t NN = (size_t)o->N * o->N;
    mw_status s = MW_OK;
    float *dv = nullptr, *dn = nullptr, *dw = nullptr;
    if (nsteps == 1) { dv = f.s_vert; dn = f.s_norm; dw = f.s_white; frame_fftmesh_overwritten(o); }  // by the launches below, whitecap stride 1
    else if ((s = dmalloc(&dv, NN * 3 * nsteps)) != MW_OK || (s = dmalloc(&dn, NN * 3 * nsteps)) != MW_OK || (s = dmalloc(&dw, NN * nsteps)) != MW_OK) {
        hipFree(dv); hipFree(dn); hipFree(dw);
        return s;
    }
    static const char* names[2] = {"k_pass1 (h~ + transform along i)", "k_pass2 (transform along j + epilogue)"};
    kt.n = 2; kt.names = names; kt.report_failed = true;
    float t[MW_MAX_BATCH];
    for (int k = 0; k < nsteps; k++) t[k] = 1.0f + (float)k / 60.f;
    auto call = [&](hipEvent_t* between) { return fm_evaluate(f, f.sp, consts_of(o), t, nsteps, dv, dn, dw, 1, o->stream, false, nullptr, between); };
    Events ev(2 * iters + 1);
    s = warm_up(o->stream, [&] { return call(nullptr); });
    hipEventRecord(ev[0], o->stream);
    for (int it = 0; it < iters && s == MW_OK; it++) {
        s = call(&ev[2 * it + 1]);
        hipEventRecord(ev[2 * it + 2], o->stream);
    }
    hipEventSynchronize(ev[2 * iters]);
    for (int it = 0; it < iters && s == MW_OK; it++) {
        float m[2] = {0.f, 0.f};
        hipEventElapsedTime(&m[0], ev[2 * it], ev[2 * it + 1]);
        hipEventElapsedTime(&m[1], ev[2 * it + 1], ev[2 * it + 2]);
        kt.add(m);
    }
    if (nsteps != 1) { hipFree(dv); hipFree(dn); hipFree(dw); }
    else if (s == MW_OK) frame_fftmesh_made(o, 1.0f, 1);  // the host-API frame is the profiled step (t = 1) now
    return s;
}
static mw_status profile_kernels_impl(mw_ocean* o, int32_t nsteps, int32_t iters, float* ms_out, float* stats_out, const char** names_out,
                                      int32_t* nkernels) {
    if (!o || !ms_out || !nkernels || iters < 1) return fail(MW_EINVAL, "mw_ocean_profile_kernels: bad argument");
    if (nsteps < 1 || nsteps > MW_MAX_BATCH) return fail(MW_EINVAL, "nsteps out of range");
    HIP_TRY(hipSetDevice(o->device));
    HIP_TRY(hipStreamSynchronize(o->stream));
    KernelTimes kt;
    const mw_status s = o->sem == MW_SEM_OCEANRENDERER ? profile_or(o, nsteps, iters, kt)
                        : !o->use_fft                  ? profile_direct(o, nsteps, iters, kt)
                                                       : profile_fft(o, nsteps, iters, kt);
    if (s == MW_OK || kt.report_failed) kt.report(iters, s == MW_OK, ms_out, stats_out, names_out, nkernels);
    return s;
}
mw_status mw_ocean_profile_kernels(mw_ocean* o, int32_t nsteps, int32_t iters, float* ms_out, const char** names_out,
                                   int32_t* nkernels) {
    if (!ms_out) return fail(MW_EINVAL, "mw_ocean_profile_kernels: bad argument");
    return profile_kernels_impl(o, nsteps, iters, ms_out, nullptr, names_out, nkernels);
}
mw_status mw_ocean_profile_kernels_stats(mw_ocean* o, int32_t nsteps, int32_t iters, float* stats_out, const char** names_out,
                                         int32_t* nkernels) {
    if (!stats_out) return fail(MW_EINVAL, "mw_ocean_profile_kernels_stats: bad argument");
    float ms[4] = {0.f, 0.f, 0.f, 0.f};
    return profile_kernels_impl(o, nsteps, iters, ms, stats_out, names_out, nkernels);
}

// test hook: omega(i,j)*t exactly as the kernels form it (bit-exactness check vs the oracle)
mw_status mw_debug_omega_t(mw_ocean* o, float t, float* out_host) {
    if (!o || !out_host) return fail(MW_EINVAL, "NULL argument");
    HIP_TRY(hipSetDevice(o->device));
    const int N = o->N;
    DevTmp<float> d;
    hipError_t e = d.alloc((size_t)N * N);
    if (e == hipSuccess) { hipLaunchKernelGGL(k_omega_t, dim3((N * N + 255) / 256), dim3(256), 0, o->stream, N, o->p.length, o->p.gravity, t, d.p); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(out_host, d.p, sizeof(float) * N * N, hipMemcpyDeviceToHost, o->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(o->stream);
    return e == hipSuccess ? MW_OK : fail(MW_EDEVICE, std::string("mw_debug_omega_t: ") + hipGetErrorString(e));
}

// test hook: one EvaluateWaves(t) that also returns hds = (d.x, d.z) exactly as the kernels hold it (S/FFTMesh.cs:247), so
// that the whitecap stage -- forward differences, the i = N-1 / j = N-1 edge rules (:258-274), the halo rows handed
// between workgroups -- can be compared BIT FOR BIT with the oracle's float32 whitecap of the same hds and normals
mw_status mw_debug_evaluate_hds(mw_ocean* o, float t, float* vertices_xyz, float* normals_xyz, float* colors_rgba, float* hds_xy) {
    if (!o || !hds_xy) return fail(MW_EINVAL, "mw_debug_evaluate_hds: NULL argument");
    if (o->sem != MW_SEM_FFTMESH) return fail(MW_ESTATE, "mw_debug_evaluate_hds: FFTMesh semantics only");
    HIP_TRY(hipSetDevice(o->device));
    const size_t NN = (size_t)o->N * o->N;
    FmState& f = o->fm;
    cf* dh = o->direct.hds;  // the direct-sum kernels leave hds there
    mw_status s = o->use_fft ? scratch_reserve(o, NN * sizeof(cf)) : mw_ocean_evaluate_device(o, &t, 1, f.s_vert, f.s_norm, f.s_white, MW_OUT_COLOR_RGBA);
    if (s == MW_OK && o->use_fft) {
        dh = static_cast<cf*>(o->scratch.p);
        s = fm_evaluate(f, f.sp, consts_of(o), &t, 1, f.s_vert, f.s_norm, f.s_white, 4, o->stream, false, dh);
    }
    if (s != MW_OK) return s;
    frame_fftmesh_made(o, t, 4);
    return fm_frame_to_host(f, NN, vertices_xyz, normals_xyz, colors_rgba, dh, hds_xy, o->stream);
}

// measurement hook: the pass-1 time group an enqueue of nsteps uses (bench.py prints what it timed)
int32_t mw_debug_pass1_time_group(mw_ocean* o, int32_t nsteps) {
    return (o && o->sem == MW_SEM_FFTMESH && o->use_fft && nsteps >= 1 && nsteps <= MW_MAX_BATCH) ? p1_time_group(o->fm, nsteps) : 0;
}

// test hooks: the stored omega table and the device sincos
__global__ void k_dbg_sincos(const float* x, int n, float* sn, float* cs) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sincos_f32(x[i], &sn[i], &cs[i]);
}
__global__ void k_dbg_sincos_fast(const float* x, int n, float* sn, float* cs) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) sincos_fast_f32(x[i], &sn[i], &cs[i]);
}
// test hook: ONE wave applies wave_transpose4 (v_permlane16_swap / v_permlane32_swap, mw_math.h) to 64 lanes x 16 complex slots
__global__ __launch_bounds__(64) void k_dbg_wave_transpose4(cf* io) {
    cf x[16];
#pragma unroll
    for (int r = 0; r < 16; r++) x[r] = io[threadIdx.x * 16 + r];
    wave_transpose4<16>(x);
#pragma unroll
    for (int r = 0; r < 16; r++) io[threadIdx.x * 16 + r] = x[r];
}
static mw_status debug_sincos(const float* x_host, int32_t n, float* s_host, float* c_host, bool fast) {
    if (!x_host || !s_host || !c_host || n < 1) return fail(MW_EINVAL, "mw_debug_sincos: bad argument");
    DevTmp<float> dc, ds, dx;  // (freed in the order dx, ds, dc)
    hipError_t e = dx.alloc((size_t)n);
    if (e == hipSuccess) e = ds.alloc((size_t)n);
    if (e == hipSuccess) e = dc.alloc((size_t)n);
    if (e == hipSuccess) e = hipMemcpy(dx.p, x_host, 4 * (size_t)n, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        if (fast) hipLaunchKernelGGL(k_dbg_sincos_fast, dim3((n + 255) / 256), dim3(256), 0, 0, dx.p, n, ds.p, dc.p);
        else hipLaunchKernelGGL(k_dbg_sincos, dim3((n + 255) / 256), dim3(256), 0, 0, dx.p, n, ds.p, dc.p);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(s_host, ds.p, 4 * (size_t)n, hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(c_host, dc.p, 4 * (size_t)n, hipMemcpyDeviceToHost);
    return e == hipSuccess ? MW_OK : fail(MW_EDEVICE, std::string("mw_debug_sincos: ") + hipGetErrorString(e));
}
mw_status mw_debug_sincos(const float* x_host, int32_t n, float* s_host, float* c_host) {
    return debug_sincos(x_host, n, s_host, c_host, false);
}
mw_status mw_debug_sincos_fast(const float* x_host, int32_t n, float* s_host, float* c_host) {
    return debug_sincos(x_host, n, s_host, c_host, true);
}
mw_status mw_debug_set_switch(const char* name, int32_t value) {
    const int k = switch_index(name);
    if (k < 0) return fail(MW_EINVAL, std::string("mw_debug_set_switch: unknown switch ") + (name ? name : "(null)"));
    switch_table().v[k].store(value);
    return MW_OK;
}
int32_t mw_debug_get_switch(const char* name) {
    const int k = switch_index(name);
    return k < 0 ? INT32_MIN : sw((Switch)k);
}
mw_status mw_debug_wave_transpose4(float* inout_host) {
    if (!inout_host) return fail(MW_EINVAL, "NULL argument");
    DevTmp<cf> d;
    hipError_t e = d.alloc(64 * 16);
    if (e == hipSuccess) e = hipMemcpy(d.p, inout_host, sizeof(cf) * 64 * 16, hipMemcpyHostToDevice);
    if (e == hipSuccess) { hipLaunchKernelGGL(k_dbg_wave_transpose4, dim3(1), dim3(64), 0, 0, d.p); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpy(inout_host, d.p, sizeof(cf) * 64 * 16, hipMemcpyDeviceToHost);
    return e == hipSuccess ? MW_OK : fail(MW_EDEVICE, std::string("mw_debug_wave_transpose4: ") + hipGetErrorString(e));
}
mw_status mw_debug_stream_read(int64_t bytes, int32_t width, int32_t iters) {
    DevTmp<float> sink;
    DevTmp<char> buf;  // (freed first)
    HIP_TRY(buf.alloc((size_t)bytes));
    HIP_TRY(sink.alloc(4096));
    HIP_TRY(hipMemset(buf.p, 0, (size_t)bytes));
    for (int it = 0; it < iters; it++) {
        if (width == 4) k_dbg_stream<float><<<2048, 256>>>((const float*)buf.p, (size_t)bytes / 4, sink.p);
        else if (width == 8) k_dbg_stream<cf><<<2048, 256>>>((const cf*)buf.p, (size_t)bytes / 8, sink.p);
        else k_dbg_stream<f4><<<2048, 256>>>((const f4*)buf.p, (size_t)bytes / 16, sink.p);
    }
    return hipDeviceSynchronize() == hipSuccess ? MW_OK : fail(MW_EDEVICE, "stream_read failed");
}

mw_status mw_debug_get_omega(mw_ocean* o, float* out_host) {  // [j][i] layout
    if (!o || !o->fm.sp.Om) return fail(MW_EINVAL, "no omega table");
    HIP_TRY(hipMemcpy(out_host, o->fm.sp.Om, sizeof(float) * o->N * o->N, hipMemcpyDeviceToHost));
    return MW_OK;
}

// test hook: the hierarchy a raycast of this frame would traverse (raycast.h), every node of every level.  The cast's own checks
// (raycast_prepare / raycast_tiled_prepare, on one ray's worth of arrays that are only tested against NULL: an OceanRenderer mesh is
// displaced only for a call that has rays) and the cast's own build (raycast_build / raycast_tiled_build).  The first build sizes the
// handle's tree buffer and names the geometry; its rc_nodes(D) boxes are then set to 0xFF bytes and built again, so that a node no
// kernel writes comes back NaN.
mw_status mw_debug_raycast_tree(mw_ocean* o, int32_t frame, int32_t tiled, float* box_host, int64_t capacity_nodes, int32_t geom[3]) {
    const char* who = "mw_debug_raycast_tree";
    if (!geom) return fail(MW_EINVAL, who, "NULL geom");
    if (o) HIP_TRY(hipSetDevice(o->device));
    SqMesh m{};
    mw_status s = tiled ? raycast_tiled_prepare(o, frame, geom, 1, 0, geom, who, &m) : raycast_prepare(o, frame, geom, 1, geom, who, &m);
    if (s != MW_OK) return s;
    RcTree tr;
    auto build = [&] { return tiled ? raycast_tiled_build(o, m, &tr) : raycast_build(o, m, &tr); };
    if ((s = build()) != MW_OK) return s;
    const size_t bytes = (size_t)rc_nodes(tr.D) * 8 * sizeof(float);
    HIP_TRY(hipMemsetAsync(tr.box, 0xFF, bytes, o->stream));
    if ((s = build()) != MW_OK) return s;
    geom[0] = tr.B; geom[1] = tr.nb; geom[2] = tr.D;
    if (box_host && capacity_nodes < rc_nodes(tr.D)) {
        HIP_TRY(hipStreamSynchronize(o->stream));
        return fail(MW_EINVAL, who, "capacity_nodes is below the tree's node count (geom[2] = D; (4^(D+1) - 1) / 3 nodes)");
    }
    if (box_host) HIP_TRY(hipMemcpyAsync(box_host, tr.box, bytes, hipMemcpyDeviceToHost, o->stream));
    HIP_TRY(hipStreamSynchronize(o->stream));
    return MW_OK;
}

// test hook: the footprint queries on a caller's mesh.  No handle: the arrays go to the device, the services' own launches
// (query_surface_launch / query_velocity_launch, surface_services.inc: k_query_surface<SqMesh>, k_query_velocity<SqMesh>) run on the null
// stream, the rows come back.  The services' argument rules (query_args_check) and the mesh rules a handle guarantees (R >= 2,
// unit_width > 0, a whitecap stride of 1 or 4), before any device call.
mw_status mw_debug_query_mesh(int32_t R, float unit_width, const float* vert, const float* norm, const float* white, int32_t wstride,
                              const float* vel, int32_t mode, int32_t iterations, const float* xz, int64_t n, float* out, float* vout) {
    const char* who = "mw_debug_query_mesh";
    if (R < 2 || R > 16384) return fail(MW_EINVAL, who, "R must be in [2, 16384]");  // 3 R^2 stays an int
    if (!(unit_width > 0.f)) return fail(MW_EINVAL, who, "the mesh needs unit_width > 0");
    if (wstride != 1 && wstride != 4) return fail(MW_EINVAL, who, "wstride must be 1 or 4");
    mw_status s = query_args_check(mode, xz, n, iterations, out, who);
    if (s != MW_OK) return s;
    if (n == 0) return MW_OK;
    if (!vert || !norm || !white) return fail(MW_EINVAL, who, "NULL mesh array");
    if (vel && !vout) return fail(MW_EINVAL, who, "vel without vout");
    const size_t nv = (size_t)R * R, nn = (size_t)n;
    DevTmp<float> dvo, dout, dxz, dvel, dwhite, dnorm, dvert;
    HIP_TRY(dvert.alloc(3 * nv));
    HIP_TRY(dnorm.alloc(3 * nv));
    HIP_TRY(dwhite.alloc((size_t)wstride * nv));
    HIP_TRY(dxz.alloc(2 * nn));
    HIP_TRY(dout.alloc(8 * nn));
    HIP_TRY(hipMemcpy(dvert.p, vert, sizeof(float) * 3 * nv, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dnorm.p, norm, sizeof(float) * 3 * nv, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dwhite.p, white, sizeof(float) * wstride * nv, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(dxz.p, xz, sizeof(float) * 2 * nn, hipMemcpyHostToDevice));
    const SqMesh m{dvert.p, dnorm.p, dwhite.p, R, wstride, unit_width, 0.f};
    if ((s = query_surface_launch(nullptr, m, mode, iterations, dxz.p, n, dout.p)) != MW_OK) return s;
    if (vel) {
        HIP_TRY(dvel.alloc(3 * nv));
        HIP_TRY(dvo.alloc(4 * nn));
        HIP_TRY(hipMemcpy(dvel.p, vel, sizeof(float) * 3 * nv, hipMemcpyHostToDevice));
        if ((s = query_velocity_launch(nullptr, m, dvel.p, mode, iterations, dxz.p, n, dvo.p)) != MW_OK) return s;
        HIP_TRY(hipMemcpy(vout, dvo.p, sizeof(float) * 4 * nn, hipMemcpyDeviceToHost));
    }
    HIP_TRY(hipMemcpy(out, dout.p, sizeof(float) * 8 * nn, hipMemcpyDeviceToHost));  // waits for the null stream
    return MW_OK;
}

#ifdef MW_TIMING
mw_status mw_debug_get_stamps(long long* out_host) {
    HIP_TRY(hipMemcpyFromSymbol(out_host, HIP_SYMBOL(g_stamps), sizeof(long long) * 2 * 64 * 16 * 32));
    return MW_OK;
}
#endif
