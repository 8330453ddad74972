// tiles.inc -- independent ocean tiles on several devices and their RCCL gather (included by mistral_water.hip inside
// extern "C").  SURVEY.md 8e: the path shards over independent units (tiles), no data-path collective; the only exchange
// is the optional gather of finished outputs, on per-device SIDE streams behind an event on the compute streams.
//
// RCCL is bound at run time (dlopen + dlsym): libmistral_water.so keeps no link-time dependency on it, single-GPU hosts
// never load it, and a process that already carries a librccl.so.1 (PyTorch bundles one) shares that copy.

namespace {

// the slice of rccl.h this file uses (/opt/rocm/include/rccl/rccl.h:187,220,236,260,339,700,722,923,930)
typedef struct ncclComm* mw_ncclComm_t;
typedef struct { char internal[MW_COMM_ID_BYTES]; } mw_ncclUniqueId;
enum { MW_NCCL_SUCCESS = 0, MW_NCCL_FLOAT32 = 7 };
struct Rccl {
    void* lib = nullptr;
    int (*GetUniqueId)(mw_ncclUniqueId*) = nullptr;
    int (*CommInitRank)(mw_ncclComm_t*, int, mw_ncclUniqueId, int) = nullptr;
    int (*CommInitAll)(mw_ncclComm_t*, int, const int*) = nullptr;
    int (*CommDestroy)(mw_ncclComm_t) = nullptr;
    int (*GroupStart)() = nullptr;
    int (*GroupEnd)() = nullptr;
    int (*Send)(const void*, size_t, int, int, mw_ncclComm_t, hipStream_t) = nullptr;
    int (*Recv)(void*, size_t, int, int, mw_ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(int) = nullptr;
};
Rccl g_rccl;
std::once_flag g_rccl_once;
std::string g_rccl_err;

const Rccl* rccl() {
    std::call_once(g_rccl_once, [] {
        const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
        for (const char* n : names)
            if ((g_rccl.lib = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
        if (!g_rccl.lib) { g_rccl_err = std::string("dlopen(librccl.so.1): ") + dlerror(); return; }
#define MW_SYM(field, sym)                                                                   \
    *reinterpret_cast<void**>(&g_rccl.field) = dlsym(g_rccl.lib, sym);                       \
    if (!g_rccl.field) { g_rccl_err = std::string("RCCL symbol missing: ") + sym; g_rccl.lib = nullptr; return; }
        MW_SYM(GetUniqueId, "ncclGetUniqueId") MW_SYM(CommInitRank, "ncclCommInitRank") MW_SYM(CommInitAll, "ncclCommInitAll")
        MW_SYM(CommDestroy, "ncclCommDestroy") MW_SYM(GroupStart, "ncclGroupStart") MW_SYM(GroupEnd, "ncclGroupEnd")
        MW_SYM(Send, "ncclSend") MW_SYM(Recv, "ncclRecv") MW_SYM(GetErrorString, "ncclGetErrorString")
#undef MW_SYM
    });
    return g_rccl.lib ? &g_rccl : nullptr;
}
#define RCCL_TRY(R, expr)                                                                                   \
    do {                                                                                                    \
        int r_ = (expr);                                                                                    \
        if (r_ != MW_NCCL_SUCCESS) return fail(MW_EDEVICE, std::string(#expr) + ": " + (R)->GetErrorString(r_)); \
    } while (0)

// The multi-device entry points walk hipSetDevice over their tiles: the caller's current device is put back on every exit
// (PyTorch in the same thread would otherwise allocate and launch on the last tile's GPU without any error).
struct DeviceGuard {
    int prev = -1;
    DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) { prev = -1; (void)hipGetLastError(); } }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

}  // namespace

struct mw_tiles {
    struct Local {
        mw_ocean* ocean = nullptr;
        int device = 0, rank = 0;  // rank = communicator rank of this tile's device
        int global_index = 0;
        // FFTMesh: TWO sets of [max_steps][...] outputs, used ping-pong by evaluate / gather (round 5): a gather sends straight from the set
        // the latest evaluate wrote and steers the NEXT evaluate to the other one -- no snapshot copy on the compute stream (round 4:
        // four hipMemcpyAsync per gather there, 11 % of the step rate at 1024^2).  Set 1 is allocated by the first gather; a job that never
        // gathers keeps one set and stable output pointers.  (OceanRenderer tiles keep their textures in the handle and snapshot them.)
        float *dv[2] = {nullptr, nullptr}, *dn[2] = {nullptr, nullptr}, *dw[2] = {nullptr, nullptr};
        int last = 0, next = 0;                             // set the latest evaluate wrote / set the next evaluate writes
        hipEvent_t sent_set[2] = {nullptr, nullptr};        // recorded on the side stream after the sends that read set k
        bool sent_pending[2] = {false, false};
        float* staged = nullptr;                            // OceanRenderer: snapshot of the gathered frame [floats_per_tile]
        // OceanRenderer tiles with max_steps > 1: the textures of every frame of the latest mw_tiles_generate_texture_steps, [max_steps][...]
        float *fh = nullptr, *fd = nullptr, *fn = nullptr, *fw = nullptr;
        int frames = 0;                                     // frames the latest call wrote there
        hipEvent_t done = nullptr;                          // recorded on the compute stream: the gathered data is complete
    };
    struct Dev {  // one per distinct local device = one communicator rank
        int device = 0, rank = 0;
        hipStream_t side = nullptr;
        hipEvent_t sent = nullptr;  // recorded on the side stream after a gather's sends: the next snapshot waits for it
        bool sent_pending = false;
        mw_ncclComm_t comm = nullptr;
    };
    std::vector<Local> tiles;
    std::vector<Dev> devs;
    std::vector<int> rank_of_tile;  // communicator rank of every tile of the JOB (global index)
    int ntiles_total = 0, nranks = 0, max_steps = 0, N = 0;
    int white_stride = 1;
    uint32_t flags = 0;
    bool multiprocess = false;
    float* gathered = nullptr;  // on the root's device, [ntiles_total][floats_per_tile]
    int gathered_device = -1;
    int sem = MW_SEM_FFTMESH;
    // what one tile contributes to a gather: FFTMesh vertices 3 + normals 3 + whitecap w floats per grid point of one step;
    // OceanRenderer the four result textures of the latest GenerateTexture(): height 1 + disp.rb 2 + normal 3 + white 1
    int nparts() const { return sem == MW_SEM_FFTMESH ? 3 : 4; }
    size_t part_count(int a) const {
        const size_t NN = (size_t)N * N;
        if (sem == MW_SEM_FFTMESH) return a < 2 ? NN * 3 : NN * (size_t)white_stride;
        const size_t c[4] = {NN, NN * 2, NN * 3, NN};
        return c[a];
    }
    size_t part_offset(int a) const { size_t o = 0; for (int b = 0; b < a; b++) o += part_count(b); return o; }
    size_t floats_per_tile() const { return part_offset(nparts()); }
    const float* part_src(const Local& L, int a, int step) const {
        if (sem == MW_SEM_FFTMESH) {
            const size_t NN = (size_t)N * N;
            const int c = L.last;
            return a == 0 ? L.dv[c] + (size_t)step * NN * 3 : (a == 1 ? L.dn[c] + (size_t)step * NN * 3 : L.dw[c] + (size_t)step * NN * white_stride);
        }
        if (L.fh) {  // frame `step` of the latest steps call
            const size_t off = (size_t)step * N * N;
            return a == 0 ? L.fh + off : (a == 1 ? L.fd + 2 * off : (a == 2 ? L.fn + 3 * off : L.fw + off));
        }
        const OrTex& s = L.ocean->orr.out;
        return a == 0 ? s.height : (a == 1 ? reinterpret_cast<const float*>(s.disp) : (a == 2 ? s.normal : s.white));
    }
    Dev* dev_of(int device) { for (auto& d : devs) if (d.device == device) return &d; return nullptr; }
};

// one set of FFTMesh outputs of a tile (vertices 3, normals 3, whitecap up to 4 floats per grid point and step) on the current device
static bool tiles_alloc_set(mw_tiles::Local& L, int c, size_t NN, int max_steps) {
    return hipMalloc((void**)&L.dv[c], sizeof(float) * NN * 3 * max_steps) == hipSuccess &&
           hipMalloc((void**)&L.dn[c], sizeof(float) * NN * 3 * max_steps) == hipSuccess &&
           hipMalloc((void**)&L.dw[c], sizeof(float) * NN * 4 * max_steps) == hipSuccess;
}
static void tiles_free_local(mw_tiles::Local& L) {
    for (int c = 0; c < 2; c++) {
        hipFree(L.dv[c]); hipFree(L.dn[c]); hipFree(L.dw[c]);
        L.dv[c] = L.dn[c] = L.dw[c] = nullptr;
        if (L.sent_set[c]) { hipEventDestroy(L.sent_set[c]); L.sent_set[c] = nullptr; }
    }
    hipFree(L.staged); L.staged = nullptr;
    hipFree(L.fh); hipFree(L.fd); hipFree(L.fn); hipFree(L.fw);
    L.fh = L.fd = L.fn = L.fw = nullptr;
    if (L.done) { hipEventDestroy(L.done); L.done = nullptr; }
    if (L.ocean) { mw_ocean_destroy(L.ocean); L.ocean = nullptr; }
}

static mw_status tiles_alloc_local(mw_tiles* t, const mw_params* params, int device, int global_index, int rank) {
    mw_params p = *params;
    p.seed = params->seed + (uint64_t)global_index;
    p.device = device;
    mw_tiles::Local L;
    L.device = device; L.rank = rank; L.global_index = global_index;
    mw_status s = mw_ocean_create(&p, &L.ocean);
    if (s != MW_OK) return s;
    t->N = L.ocean->N;
    t->sem = L.ocean->sem;
    const size_t NN = (size_t)t->N * t->N;
    const bool fm = (t->sem == MW_SEM_FFTMESH);
    if ((fm && !tiles_alloc_set(L, 0, NN, t->max_steps)) ||
        (!fm && hipMalloc((void**)&L.staged, sizeof(float) * NN * 7) != hipSuccess) ||
        (!fm && t->max_steps > 1 && (hipMalloc((void**)&L.fh, sizeof(float) * NN * t->max_steps) != hipSuccess ||
                                     hipMalloc((void**)&L.fd, sizeof(float) * NN * 2 * t->max_steps) != hipSuccess ||
                                     hipMalloc((void**)&L.fn, sizeof(float) * NN * 3 * t->max_steps) != hipSuccess ||
                                     hipMalloc((void**)&L.fw, sizeof(float) * NN * t->max_steps) != hipSuccess)) ||
        hipEventCreateWithFlags(&L.done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&L.sent_set[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&L.sent_set[1], hipEventDisableTiming) != hipSuccess) {
        tiles_free_local(L);
        return fail(MW_ENOMEM, "mw_tiles: output buffers of a tile could not be allocated");
    }
    t->tiles.push_back(L);
    return MW_OK;
}

mw_status mw_comm_unique_id(void* id_out) {
    if (!id_out) return fail(MW_EINVAL, "mw_comm_unique_id: NULL argument");
    const Rccl* R = rccl();
    if (!R) return fail(MW_EDEVICE, "RCCL is not available: " + g_rccl_err);
    mw_ncclUniqueId id;
    RCCL_TRY(R, R->GetUniqueId(&id));
    std::memcpy(id_out, &id, MW_COMM_ID_BYTES);
    return MW_OK;
}

void mw_tiles_destroy(mw_tiles* t) {
    if (!t) return;
    DeviceGuard guard;
    for (auto& L : t->tiles) {
        hipSetDevice(L.device);
        if (L.ocean) hipStreamSynchronize(L.ocean->stream);
    }
    for (auto& d : t->devs) {
        hipSetDevice(d.device);
        if (d.side) hipStreamSynchronize(d.side);
        if (d.comm && rccl()) rccl()->CommDestroy(d.comm);
        if (d.sent) hipEventDestroy(d.sent);
        if (d.side) hipStreamDestroy(d.side);
    }
    if (t->gathered) { hipSetDevice(t->gathered_device); hipFree(t->gathered); }
    for (auto& L : t->tiles) {
        hipSetDevice(L.device);
        tiles_free_local(L);
    }
    delete t;
}

static mw_status tiles_check(const mw_params* params, int32_t max_steps, mw_tiles** out) {
    if (!params || !out) return fail(MW_EINVAL, "mw_tiles_create: NULL argument");
    *out = nullptr;
    if (params->semantics != MW_SEM_FFTMESH && params->semantics != MW_SEM_OCEANRENDERER) return fail(MW_EINVAL, "mw_tiles: unknown semantics");
    // OceanRenderer tiles: max_steps consecutive frames per mw_tiles_generate_texture_steps (the phase chain of F/FFTCommon.cginc:101-104 is
    // walked inside the spectrum kernel, mw_ocean_generate_texture_steps_device)
    if (max_steps < 1 || max_steps > (params->semantics == MW_SEM_OCEANRENDERER ? MW_OR_MAX_FRAMES : MW_MAX_BATCH))
        return fail(MW_EINVAL, "mw_tiles_create: max_steps out of range");
    return MW_OK;
}

mw_status mw_tiles_create(const mw_params* params, int32_t ntiles, const int32_t* devices, int32_t max_steps, mw_tiles** out) {
    DeviceGuard guard;
    mw_status s = tiles_check(params, max_steps, out);
    if (s != MW_OK) return s;
    const int ndev = mw_device_count();
    if (ndev < 1) return fail(MW_EDEVICE, "mw_tiles_create: no HIP device visible (this library has no CPU fallback)");
    if (ntiles < 1 || ntiles > 64) return fail(MW_EINVAL, "mw_tiles_create: ntiles must be in [1,64]");
    mw_tiles* t = new (std::nothrow) mw_tiles();
    if (!t) return fail(MW_ENOMEM, "mw_tiles_create: out of host memory");
    t->max_steps = max_steps; t->ntiles_total = ntiles;
    for (int k = 0; k < ntiles; k++) {
        const int dev = devices ? devices[k] : k % ndev;
        if (dev < 0 || dev >= ndev) { mw_tiles_destroy(t); return fail(MW_EINVAL, "mw_tiles_create: bad device ordinal"); }
        if (!t->dev_of(dev)) { mw_tiles::Dev d; d.device = dev; d.rank = (int)t->devs.size(); t->devs.push_back(d); }
        const int rank = t->dev_of(dev)->rank;
        t->rank_of_tile.push_back(rank);
        if ((s = tiles_alloc_local(t, params, dev, k, rank)) != MW_OK) { mw_tiles_destroy(t); return s; }
    }
    t->nranks = (int)t->devs.size();
    for (auto& d : t->devs) {
        if (hipSetDevice(d.device) != hipSuccess || hipStreamCreateWithFlags(&d.side, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&d.sent, hipEventDisableTiming) != hipSuccess) {
            mw_tiles_destroy(t);
            return fail(MW_EDEVICE, "mw_tiles_create: side stream creation failed");
        }
    }
    // one communicator rank per distinct device (a single device gets a 1-rank communicator: its gather is an RCCL
    // self send/receive, so the same code path runs on a 1-GPU box)
    const Rccl* R = rccl();
    if (!R) { mw_tiles_destroy(t); return fail(MW_EDEVICE, "RCCL is not available: " + g_rccl_err); }
    std::vector<int> devlist;
    for (auto& d : t->devs) devlist.push_back(d.device);
    std::vector<mw_ncclComm_t> comms(devlist.size(), nullptr);
    int r = R->CommInitAll(comms.data(), (int)devlist.size(), devlist.data());
    if (r != MW_NCCL_SUCCESS) { mw_tiles_destroy(t); return fail(MW_EDEVICE, std::string("ncclCommInitAll: ") + R->GetErrorString(r)); }
    for (size_t i = 0; i < comms.size(); i++) t->devs[i].comm = comms[i];
    *out = t;
    return MW_OK;
}

mw_status mw_tiles_create_rank(const mw_params* params, int32_t device, int32_t max_steps, const void* comm_id, int32_t rank,
                               int32_t nranks, mw_tiles** out) {
    mw_status s = tiles_check(params, max_steps, out);
    if (s != MW_OK) return s;
    if (!comm_id || nranks < 1 || rank < 0 || rank >= nranks) return fail(MW_EINVAL, "mw_tiles_create_rank: bad rank / comm id");
    DeviceGuard guard;
    const int ndev = mw_device_count();
    if (device < 0 || device >= ndev) return fail(ndev ? MW_EINVAL : MW_EDEVICE, "mw_tiles_create_rank: bad device ordinal");
    const Rccl* R = rccl();
    if (!R) return fail(MW_EDEVICE, "RCCL is not available: " + g_rccl_err);
    mw_tiles* t = new (std::nothrow) mw_tiles();
    if (!t) return fail(MW_ENOMEM, "mw_tiles_create_rank: out of host memory");
    t->max_steps = max_steps; t->ntiles_total = nranks; t->nranks = nranks; t->multiprocess = true;
    for (int k = 0; k < nranks; k++) t->rank_of_tile.push_back(k);  // tile k lives on rank k
    if ((s = tiles_alloc_local(t, params, device, rank, rank)) != MW_OK) { mw_tiles_destroy(t); return s; }
    mw_tiles::Dev d;
    d.device = device; d.rank = rank;
    if (hipSetDevice(device) != hipSuccess || hipStreamCreateWithFlags(&d.side, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&d.sent, hipEventDisableTiming) != hipSuccess) {
        mw_tiles_destroy(t);
        return fail(MW_EDEVICE, "mw_tiles_create_rank: side stream creation failed");
    }
    mw_ncclUniqueId id;
    std::memcpy(&id, comm_id, MW_COMM_ID_BYTES);
    int r = R->CommInitRank(&d.comm, nranks, id, rank);
    t->devs.push_back(d);
    if (r != MW_NCCL_SUCCESS) { mw_tiles_destroy(t); return fail(MW_EDEVICE, std::string("ncclCommInitRank: ") + R->GetErrorString(r)); }
    *out = t;
    return MW_OK;
}

int32_t mw_tiles_count(const mw_tiles* t) { return t ? t->ntiles_total : 0; }
int32_t mw_tiles_local_count(const mw_tiles* t) { return t ? (int32_t)t->tiles.size() : 0; }
mw_ocean* mw_tiles_ocean(mw_tiles* t, int32_t k) { return (t && k >= 0 && k < (int)t->tiles.size()) ? t->tiles[k].ocean : nullptr; }

mw_status mw_tiles_generate_texture_steps(mw_tiles* t, const float* delta_time, int32_t nframes) {
    if (!t || !delta_time) return fail(MW_EINVAL, "mw_tiles_generate_texture_steps: NULL argument");
    if (t->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, "mw_tiles_generate_texture_steps: OceanRenderer tiles only (FFTMesh tiles: mw_tiles_evaluate)");
    if (nframes < 1 || nframes > t->max_steps) return fail(MW_EINVAL, "mw_tiles_generate_texture_steps: nframes out of range (max_steps of mw_tiles_create)");
    DeviceGuard guard;
    for (auto& L : t->tiles) {  // asynchronous: nframes consecutive GenerateTexture() calls per tile in one enqueue, every device works at once
        mw_status s = mw_ocean_generate_texture_steps_device(L.ocean, delta_time, nframes, L.fh, L.fd, L.fn, L.fw);
        if (s != MW_OK) return s;
        L.frames = nframes;
    }
    return MW_OK;
}
mw_status mw_tiles_generate_texture(mw_tiles* t, float delta_time) {
    if (!t) return fail(MW_EINVAL, "mw_tiles_generate_texture: NULL handle");
    return mw_tiles_generate_texture_steps(t, &delta_time, 1);
}
mw_status mw_tiles_frames(mw_tiles* t, int32_t k, void** d_height, void** d_disp_xz, void** d_normal_xyz, void** d_white) {
    if (!t || k < 0 || k >= (int)t->tiles.size()) return fail(MW_EINVAL, "mw_tiles_frames: bad tile index");
    if (t->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, "mw_tiles_frames: OceanRenderer tiles only (FFTMesh tiles: mw_tiles_outputs)");
    const mw_tiles::Local& L = t->tiles[k];
    if (!L.fh) return fail(MW_ESTATE, "mw_tiles_frames: tiles created with max_steps 1 keep one frame (mw_tiles_textures)");
    if (d_height) *d_height = L.fh;
    if (d_disp_xz) *d_disp_xz = L.fd;
    if (d_normal_xyz) *d_normal_xyz = L.fn;
    if (d_white) *d_white = L.fw;
    return MW_OK;
}

mw_status mw_tiles_textures(mw_tiles* t, int32_t k, void** d_height, void** d_disp_xz, void** d_normal_xyz, void** d_white) {
    if (!t || k < 0 || k >= (int)t->tiles.size()) return fail(MW_EINVAL, "mw_tiles_textures: bad tile index");
    if (t->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, "mw_tiles_textures: OceanRenderer tiles only (FFTMesh tiles: mw_tiles_outputs)");
    const OrTex& s = t->tiles[k].ocean->orr.out;
    if (d_height) *d_height = s.height;
    if (d_disp_xz) *d_disp_xz = s.disp;
    if (d_normal_xyz) *d_normal_xyz = s.normal;
    if (d_white) *d_white = s.white;
    return MW_OK;
}

mw_status mw_tiles_evaluate(mw_tiles* t, const float* times, int32_t nsteps, uint32_t flags) {
    if (!t || !times) return fail(MW_EINVAL, "mw_tiles_evaluate: NULL argument");
    if (t->sem != MW_SEM_FFTMESH) return fail(MW_ESTATE, "mw_tiles_evaluate: FFTMesh tiles only (OceanRenderer tiles: mw_tiles_generate_texture)");
    if (nsteps < 1 || nsteps > t->max_steps) return fail(MW_EINVAL, "mw_tiles_evaluate: nsteps out of range");
    DeviceGuard guard;
    t->flags = flags;
    t->white_stride = (flags & MW_OUT_COLOR_RGBA) ? 4 : 1;
    for (auto& L : t->tiles) {  // asynchronous: one enqueue per tile, every device works at once
        const int c = L.next;
        if (L.sent_pending[c]) {  // the sends of the gather that read this set (two enqueues ago) must be done before it is overwritten
            HIP_TRY(hipSetDevice(L.device));
            HIP_TRY(hipStreamWaitEvent(L.ocean->stream, L.sent_set[c], 0));
            L.sent_pending[c] = false;
        }
        mw_status s = mw_ocean_evaluate_device(L.ocean, times, nsteps, L.dv[c], L.dn[c], L.dw[c], flags);
        if (s != MW_OK) return s;
        L.last = c;
    }
    return MW_OK;
}

mw_status mw_tiles_outputs(mw_tiles* t, int32_t k, void** d_vertices, void** d_normals, void** d_white) {
    if (!t || k < 0 || k >= (int)t->tiles.size()) return fail(MW_EINVAL, "mw_tiles_outputs: bad tile index");
    if (t->sem != MW_SEM_FFTMESH) return fail(MW_ESTATE, "mw_tiles_outputs: FFTMesh tiles only (OceanRenderer tiles: mw_tiles_textures)");
    const mw_tiles::Local& L = t->tiles[k];  // the set the latest mw_tiles_evaluate wrote (the sets alternate once gathers are in use)
    if (d_vertices) *d_vertices = L.dv[L.last];
    if (d_normals) *d_normals = L.dn[L.last];
    if (d_white) *d_white = L.dw[L.last];
    return MW_OK;
}

mw_status mw_tiles_gather(mw_tiles* t, int32_t step, int32_t root) {
    if (!t) return fail(MW_EINVAL, "NULL handle");
    if (step < 0 || step >= t->max_steps || root < 0 || root >= t->ntiles_total) return fail(MW_EINVAL, "mw_tiles_gather: bad step / root");
    if (t->sem == MW_SEM_OCEANRENDERER)
        for (auto& L : t->tiles)
            if (L.fh && step >= L.frames) return fail(MW_EINVAL, "mw_tiles_gather: the latest mw_tiles_generate_texture_steps wrote fewer frames than `step`");
    const Rccl* R = rccl();
    if (!R) return fail(MW_EDEVICE, "RCCL is not available: " + g_rccl_err);
    if (t->sem == MW_SEM_OCEANRENDERER)
        for (auto& L : t->tiles)
            if (!L.ocean->orr.have_frame) return fail(MW_ESTATE, "mw_tiles_gather: no GenerateTexture() yet");
    DeviceGuard guard;
    const size_t NN = (size_t)t->N * t->N, fpt = t->floats_per_tile();
    const int np = t->nparts();
    const int root_rank = t->rank_of_tile[root];
    mw_tiles::Dev* rootdev = nullptr;
    for (auto& d : t->devs) if (d.rank == root_rank) rootdev = &d;
    if (rootdev && (!t->gathered || t->gathered_device != rootdev->device)) {
        if (t->gathered) { HIP_TRY(hipSetDevice(t->gathered_device)); HIP_TRY(hipFree(t->gathered)); t->gathered = nullptr; }
        HIP_TRY(hipSetDevice(rootdev->device));
        if (hipMalloc((void**)&t->gathered, sizeof(float) * (size_t)t->ntiles_total * (size_t)NN * 10) != hipSuccess)
            return fail(MW_ENOMEM, "mw_tiles_gather: root buffer");
        t->gathered_device = rootdev->device;
    }
    const bool fm = (t->sem == MW_SEM_FFTMESH);
    // FFTMesh tiles: NO copy on the compute stream.  An event behind the evaluate that wrote the set, the side stream waits for it and
    // sends straight from the set; the next evaluate goes to the OTHER set (allocated here on first use) and only an evaluate that comes
    // back to this set -- two enqueues later -- waits for these sends.  OceanRenderer tiles (one frame per call, textures inside the
    // handle) keep the snapshot: a 28-MB device copy per frame, then the send of the snapshot.
    for (auto& L : t->tiles) {
        HIP_TRY(hipSetDevice(L.device));
        mw_tiles::Dev* d = t->dev_of(L.device);
        hipStream_t cs = L.ocean->stream;
        if (fm) {
            const int o = L.last ^ 1;
            if (!L.dv[o] && !tiles_alloc_set(L, o, NN, t->max_steps)) {
                hipFree(L.dv[o]); hipFree(L.dn[o]); hipFree(L.dw[o]);
                L.dv[o] = L.dn[o] = L.dw[o] = nullptr;
                (void)hipGetLastError();
                return fail(MW_ENOMEM, "mw_tiles_gather: second output set of a tile could not be allocated");
            }
        } else {
            if (d->sent_pending) HIP_TRY(hipStreamWaitEvent(cs, d->sent, 0));
            for (int a = 0; a < np; a++)
                HIP_TRY(hipMemcpyAsync(L.staged + t->part_offset(a), t->part_src(L, a, step), t->part_count(a) * sizeof(float), hipMemcpyDeviceToDevice, cs));
        }
        HIP_TRY(hipEventRecord(L.done, cs));
        HIP_TRY(hipStreamWaitEvent(d->side, L.done, 0));
    }
    // One RCCL group.  A failing Send / Recv must not leave the thread's group open (every later RCCL call of this thread --
    // torch's included -- would queue behind it for ever): remember the first error, always end the group, then report.
    // Tiles that already live on the root's device do not travel: their step is copied into the root buffer on that device's side
    // stream (device-local, no communicator: round 4 sent them to themselves through RCCL, whose copy kernel held CUs for the length of
    // a 29-MB transfer -- on one device the gather cost 11 % of the step rate, 7 % once the snapshot was gone; profiles/r05_ab_notes.md).
    // RCCL carries what crosses devices, which is what it is for.
    // (switch MW_TILES_FORCE_RCCL = 1: every tile goes through ncclSend / ncclRecv, the root's own included -- how the GPU tests keep
    // the communicator path exercised on a 1-GPU box)
    const bool force_rccl = sw(SW_TILES_FORCE_RCCL) != 0;
    auto stays_home = [&](const mw_tiles::Local& L) { return !force_rccl && rootdev != nullptr && L.device == rootdev->device; };
    // (a blit kernel: the SDMA engines -- hipMemcpyDeviceToDeviceNoCU -- measured slower, with-gather 0.858 of without against 0.948)
    const hipMemcpyKind home_kind = hipMemcpyDeviceToDevice;
    for (auto& L : t->tiles) {
        if (!stays_home(L)) continue;
        HIP_TRY(hipSetDevice(L.device));
        float* dst = t->gathered + (size_t)L.global_index * fpt;
        for (int a = 0; a < np; a++)
            HIP_TRY(hipMemcpyAsync(dst + t->part_offset(a), fm ? t->part_src(L, a, step) : L.staged + t->part_offset(a), t->part_count(a) * sizeof(float),
                                   home_kind, rootdev->side));
    }
    int first_err = MW_NCCL_SUCCESS;
    const char* first_what = nullptr;
    RCCL_TRY(R, R->GroupStart());
    for (auto& L : t->tiles) {  // sends of the local tiles that cross devices (the parts of each in a fixed order)
        if (stays_home(L)) continue;
        mw_tiles::Dev* d = t->dev_of(L.device);
        for (int a = 0; a < np && first_err == MW_NCCL_SUCCESS; a++) {
            first_err = R->Send(fm ? t->part_src(L, a, step) : L.staged + t->part_offset(a), t->part_count(a), MW_NCCL_FLOAT32, root_rank, d->comm, d->side);
            if (first_err != MW_NCCL_SUCCESS) first_what = "ncclSend";
        }
    }
    if (rootdev) {  // receives on the root: tiles in global order; tiles of one rank arrive in that rank's send order
        for (int k = 0; k < t->ntiles_total && first_err == MW_NCCL_SUCCESS; k++) {
            if (!force_rccl && t->rank_of_tile[k] == root_rank) continue;  // a tile of the root's own rank = of the root's device: copied above
            float* dst = t->gathered + (size_t)k * fpt;
            for (int a = 0; a < np && first_err == MW_NCCL_SUCCESS; a++) {
                first_err = R->Recv(dst + t->part_offset(a), t->part_count(a), MW_NCCL_FLOAT32, t->rank_of_tile[k], rootdev->comm, rootdev->side);
                if (first_err != MW_NCCL_SUCCESS) first_what = "ncclRecv";
            }
        }
    }
    const int end_err = R->GroupEnd();
    // Bookkeeping first, error report after: sends and home copies may already sit on the side streams whatever RCCL returned, and the set
    // they read must not be handed to the next evaluate before they are done.  An event that cannot be recorded is replaced by waiting.
    for (auto& d : t->devs) {
        if (hipSetDevice(d.device) == hipSuccess && hipEventRecord(d.sent, d.side) == hipSuccess) d.sent_pending = true;
        else { (void)hipGetLastError(); (void)hipStreamSynchronize(d.side); }
    }
    if (fm)
        for (auto& L : t->tiles) {  // the set just sent is busy until its sends are done; the next evaluate writes the other one
            mw_tiles::Dev* d = t->dev_of(L.device);
            if (hipSetDevice(L.device) == hipSuccess && hipEventRecord(L.sent_set[L.last], d->side) == hipSuccess) L.sent_pending[L.last] = true;
            else { (void)hipGetLastError(); (void)hipStreamSynchronize(d->side); }
            L.next = L.last ^ 1;
        }
    if (first_err != MW_NCCL_SUCCESS) return fail(MW_EDEVICE, std::string(first_what) + ": " + R->GetErrorString(first_err));
    if (end_err != MW_NCCL_SUCCESS) return fail(MW_EDEVICE, std::string("ncclGroupEnd: ") + R->GetErrorString(end_err));
    return MW_OK;
}

mw_status mw_tiles_gathered(mw_tiles* t, void** d_gathered, int64_t* floats_per_tile) {
    if (!t) return fail(MW_EINVAL, "NULL handle");
    if (d_gathered) *d_gathered = t->gathered;
    if (floats_per_tile) *floats_per_tile = (int64_t)t->floats_per_tile();
    return MW_OK;
}

mw_status mw_tiles_synchronize(mw_tiles* t) {
    if (!t) return fail(MW_EINVAL, "NULL handle");
    DeviceGuard guard;
    for (auto& L : t->tiles) { HIP_TRY(hipSetDevice(L.device)); HIP_TRY(hipStreamSynchronize(L.ocean->stream)); }
    for (auto& d : t->devs) { HIP_TRY(hipSetDevice(d.device)); HIP_TRY(hipStreamSynchronize(d.side)); }
    return MW_OK;
}
