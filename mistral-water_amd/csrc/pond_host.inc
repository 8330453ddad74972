// pond_host.inc -- the handle-less entry points: Gerstner displacement and the pond material's Displacement() (included by
// mistral_water.hip inside extern "C").  Device forms launch on the caller's stream; host forms stage their arrays and run the device form.

// Device staging of the host forms: one grow-only buffer per device, held under that device's mutex for the whole (synchronous)
// call -- no hipMalloc / hipFree per frame, like the handle entry points (scratch_reserve).
static std::mutex g_pond_mu[64];
static GrowBuf g_pond_buf[64];
// grow-only; growing waits for the device before the old buffer goes.  NULL: hipMalloc failed (error cleared, the caller reports MW_ENOMEM)
static void* pond_reserve(GrowBuf& b, size_t bytes) {
    if (b.cap < bytes) {
        if (b.p) { (void)hipDeviceSynchronize(); (void)hipFree(b.p); b = GrowBuf(); }
        if (hipMalloc(&b.p, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        b.cap = bytes;
    }
    return b.p;
}
// what both host forms ask for: a visible device, a valid ordinal, nverts >= 0 (0 is the caller's no-op)
static mw_status host_form_check(const char* who, int32_t device, int64_t nverts) {
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) return fail(MW_EDEVICE, who, "no HIP device visible (no CPU fallback)");
    if (device < 0 || device >= ndev) return fail(MW_EINVAL, "bad device ordinal");
    if (nverts < 0) return fail(MW_EINVAL, "nverts < 0");
    return MW_OK;
}
// A host form once its arguments stand: positions in, displaced vertices (and normals, if wanted) out, [nverts][3] floats each, 256-byte
// aligned in the device's staging buffer; device_form(dp, dq, dn) runs the device form of the same name on the NULL stream.
static mw_status displace_staged(const char* who, int32_t device, int64_t nverts, const float* pos_xyz, float* out_xyz, float* out_normal_xyz,
                                 const std::function<mw_status(float*, float*, float*)>& device_form) {
    HIP_TRY(hipSetDevice(device));
    const size_t bytes = (size_t)nverts * 3 * sizeof(float), stride = align256(bytes);
    std::lock_guard<std::mutex> lk(g_pond_mu[device & 63]);
    char* base = static_cast<char*>(pond_reserve(g_pond_buf[device & 63], (out_normal_xyz ? 3 : 2) * stride));
    if (!base) return fail(MW_ENOMEM, who, "device staging buffer");
    float *dp = reinterpret_cast<float*>(base), *dq = reinterpret_cast<float*>(base + stride);
    float* dn = out_normal_xyz ? reinterpret_cast<float*>(base + 2 * stride) : nullptr;
    HIP_TRY(hipMemcpy(dp, pos_xyz, bytes, hipMemcpyHostToDevice));
    mw_status s = device_form(dp, dq, dn);
    if (s != MW_OK) return s;
    HIP_TRY(hipStreamSynchronize(nullptr));
    HIP_TRY(hipMemcpy(out_xyz, dq, bytes, hipMemcpyDeviceToHost));
    if (dn) HIP_TRY(hipMemcpy(out_normal_xyz, dn, bytes, hipMemcpyDeviceToHost));
    return MW_OK;
}

mw_status mw_gerstner_displace_device(const void* d_pos_xyz, int64_t nverts, const float* waves, int32_t nwaves,
                                      float amplitude, float frequency, float steepness, float t, void* d_out_xyz,
                                      void* hip_stream) {
    if (!d_pos_xyz || !d_out_xyz || !waves) return fail(MW_EINVAL, "mw_gerstner_displace_device: NULL argument");
    if (nwaves < 1 || nwaves > MW_GERSTNER_MAX_WAVES) return fail(MW_EINVAL, "nwaves must be in [1,16]");
    if (nverts < 0) return fail(MW_EINVAL, "nverts < 0");
    if (nverts == 0) return MW_OK;
    hipError_t e = gerstner_launch((const float*)d_pos_xyz, nverts, waves, nwaves, amplitude, frequency, steepness, t,
                                   (float*)d_out_xyz, reinterpret_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail(MW_EDEVICE, std::string("gerstner launch: ") + hipGetErrorString(e));
    return MW_OK;
}

int32_t mw_gerstner_max_steps(int32_t nwaves) {
    if (nwaves != 4 && nwaves != 8) return 0;
    const int m = MW_GERSTNER_PHASES / nwaves;
    return m < 32 ? m : 32;
}

mw_status mw_gerstner_displace_steps_device(const void* d_pos_xyz, int64_t nverts, const float* waves, int32_t nwaves,
                                            float amplitude, float frequency, float steepness, const float* t,
                                            int32_t nsteps, void* d_out_xyz, void* hip_stream) {
    if (!d_pos_xyz || !d_out_xyz || !waves || !t) return fail(MW_EINVAL, "mw_gerstner_displace_steps_device: NULL argument");
    const int maxs = mw_gerstner_max_steps(nwaves);
    if (maxs == 0) return fail(MW_EINVAL, "mw_gerstner_displace_steps_device: nwaves must be 4 or 8");
    if (nsteps < 1 || nsteps > maxs) return fail(MW_EINVAL, "mw_gerstner_displace_steps_device: nsteps out of range");
    if (nverts < 0) return fail(MW_EINVAL, "nverts < 0");
    if (nverts == 0) return MW_OK;
    hipError_t e = gerstner_launch_steps((const float*)d_pos_xyz, nverts, waves, nwaves, amplitude, frequency, steepness, t, nsteps,
                                         (float*)d_out_xyz, reinterpret_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail(MW_EDEVICE, std::string("gerstner launch: ") + hipGetErrorString(e));
    return MW_OK;
}

mw_status mw_gerstner_displace(const float* pos_xyz, int64_t nverts, const float* waves, int32_t nwaves, float amplitude,
                               float frequency, float steepness, float t, float* out_xyz, int32_t device) {
    if (!pos_xyz || !out_xyz || !waves) return fail(MW_EINVAL, "mw_gerstner_displace: NULL argument");
    mw_status s = host_form_check("mw_gerstner_displace", device, nverts);
    if (s != MW_OK || nverts == 0) return s;
    return displace_staged("mw_gerstner_displace", device, nverts, pos_xyz, out_xyz, nullptr, [&](float* dp, float* dq, float*) {
        return mw_gerstner_displace_device(dp, nverts, waves, nwaves, amplitude, frequency, steepness, t, dq, nullptr);
    });
}

static mw_status pond_params_of(const mw_pond_params* p, PondParams* P, const char* who) {
    if (!p) return fail(MW_EINVAL, who, "NULL params");
    if (p->mode != MW_POND_WAVE && p->mode != MW_POND_GERSTNER && p->mode != MW_POND_GERSTNER_LEVEL_ONE)
        return fail(MW_EINVAL, who, "unknown displacement mode");
    P->mode = p->mode; P->amplitude = p->amplitude; P->frequency = p->frequency; P->speed = p->speed;
    P->steepness = p->steepness; P->smoothing = p->smoothing;
    for (int i = 0; i < 4; i++) { P->wspeed[i] = p->wspeed[i]; P->dir_ab[i] = p->dir_ab[i]; P->dir_cd[i] = p->dir_cd[i]; }
    return MW_OK;
}

mw_status mw_pond_displace_device(const mw_pond_params* p, const void* d_pos_xyz, int64_t nverts, float t, void* d_out_xyz,
                                  void* d_out_normal_xyz, void* hip_stream) {
    PondParams P;
    mw_status s = pond_params_of(p, &P, "mw_pond_displace_device");
    if (s != MW_OK) return s;
    if (nverts < 0) return fail(MW_EINVAL, "nverts < 0");
    if (nverts == 0) return MW_OK;
    if (!d_pos_xyz || !d_out_xyz) return fail(MW_EINVAL, "mw_pond_displace_device: NULL argument");
    hipError_t e = pond_launch(P, (const float*)d_pos_xyz, nverts, t, (float*)d_out_xyz, (float*)d_out_normal_xyz,
                               reinterpret_cast<hipStream_t>(hip_stream));
    if (e != hipSuccess) return fail(MW_EDEVICE, std::string("pond launch: ") + hipGetErrorString(e));
    return MW_OK;
}

mw_status mw_pond_displace(const mw_pond_params* p, const float* pos_xyz, int64_t nverts, float t, float* out_xyz,
                           float* out_normal_xyz, int32_t device) {
    PondParams P;
    mw_status s = pond_params_of(p, &P, "mw_pond_displace");
    if (s != MW_OK || (s = host_form_check("mw_pond_displace", device, nverts)) != MW_OK || nverts == 0) return s;
    if (!pos_xyz || !out_xyz) return fail(MW_EINVAL, "mw_pond_displace: NULL argument");
    return displace_staged("mw_pond_displace", device, nverts, pos_xyz, out_xyz, out_normal_xyz,
                           [&](float* dp, float* dq, float* dn) { return mw_pond_displace_device(p, dp, nverts, t, dq, dn, nullptr); });
}
