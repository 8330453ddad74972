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
    struct Sent { hipEvent_t ev = nullptr; bool pending = false; };  // recorded on a side stream behind a gather's sends
    // one set of a tile's FFTMesh outputs, [max_steps][...]: vertices 3, normals 3, whitecap up to 4 floats per grid point
    struct OutSet { float *v = nullptr, *n = nullptr, *w = nullptr; Sent sent; };
    struct Local {
        mw_ocean* ocean = nullptr;
        int device = 0, global_index = 0;
        // FFTMesh: TWO sets of outputs, used ping-pong by evaluate / gather (round 5): a gather sends straight from the set
        // the latest evaluate wrote and steers the NEXT evaluate to the other one -- no snapshot copy on the compute stream (round 4:
        // four hipMemcpyAsync per gather there, 11 % of the step rate at 1024^2).  Set 1 is allocated by the first gather; a job that never
        // gathers keeps one set and stable output pointers.  (OceanRenderer tiles keep their textures in the handle and snapshot them.)
        OutSet set[2];
        int last = 0, next = 0;  // set the latest evaluate wrote / set the next evaluate writes
        float* staged = nullptr;  // OceanRenderer: snapshot of the gathered frame [floats_per_tile]
        // OceanRenderer tiles with max_steps > 1: the textures of every frame of the latest mw_tiles_generate_texture_steps, [max_steps][...]
        OrFrame fr = {};
        int frames = 0;  // frames the latest call wrote there
        hipEvent_t done = nullptr;  // recorded on the compute stream: the gathered data is complete
    };
    struct Dev {  // one per distinct local device = one communicator rank
        int device = 0, rank = 0;
        hipStream_t side = nullptr;
        Sent sent;  // the next snapshot waits for it
        mw_ncclComm_t comm = nullptr;
    };
    std::vector<Local> tiles;
    std::vector<Dev> devs;
    std::vector<int> rank_of_tile;  // communicator rank of every tile of the JOB (global index)
    int ntiles_total = 0, max_steps = 0, N = 0;
    int white_stride = 1;
    float* gathered = nullptr;  // on the root's device, [ntiles_total][floats_per_tile]
    int gathered_device = -1;
    int sem = MW_SEM_FFTMESH;
    bool fm() const { return sem == MW_SEM_FFTMESH; }
    // what one tile contributes to a gather: FFTMesh vertices 3 + normals 3 + whitecap w floats per grid point of one step;
    // OceanRenderer the four result textures of the latest GenerateTexture(): height 1 + disp.rb 2 + normal 3 + white 1
    int nparts() const { return sem == MW_SEM_FFTMESH ? 3 : 4; }
    size_t part_count(int a) const {
        const size_t v[3] = {3, 3, (size_t)white_stride}, orr[4] = {1, 2, 3, 1};
        return (size_t)N * N * (fm() ? v[a] : orr[a]);
    }
    size_t part_offset(int a) const { size_t o = 0; for (int b = 0; b < a; b++) o += part_count(b); return o; }
    size_t floats_per_tile() const { return part_offset(nparts()); }
    // part a of step `step`, where the latest evaluate, steps call or (step 0) GenerateTexture() left it
    const float* part_src(const Local& L, int a, int step) const {
        const OutSet& s = L.set[L.last];
        const float* const v[3] = {s.v, s.n, s.w};
        if (fm()) return v[a] + (size_t)step * part_count(a);
        const OrFrame f = L.fr.height ? L.fr : or_frame(L.ocean->orr, -1);
        const float* const orr[4] = {f.height, reinterpret_cast<const float*>(f.disp), f.normal, f.white};
        return orr[a] + (size_t)step * part_count(a);
    }
    // what a tile sends: FFTMesh the set itself, OceanRenderer the snapshot
    const float* send_src(const Local& L, int a, int step) const { return fm() ? part_src(L, a, step) : L.staged + part_offset(a); }
    Dev* dev_of(int device) { for (auto& d : devs) if (d.device == device) return &d; return nullptr; }
};

// Every device buffer of a tile: its pointer in Local, floats per grid point (and step, the snapshot excepted) and what
// brings it: creating an FFTMesh tile, its first gather, creating an OceanRenderer tile, and one with max_steps > 1.
enum { TILE_SET0 = 1, TILE_SET1 = 2, TILE_OR = 4, TILE_OR_STEPS = 8 };
#define AT(member) offsetof(mw_tiles::Local, member)
static const struct { size_t at; int floats, when; } tile_bufs[] = {
    {AT(set[0].v), 3, TILE_SET0}, {AT(set[0].n), 3, TILE_SET0}, {AT(set[0].w), 4, TILE_SET0},
    {AT(set[1].v), 3, TILE_SET1}, {AT(set[1].n), 3, TILE_SET1}, {AT(set[1].w), 4, TILE_SET1},
    {AT(staged), 7, TILE_OR}, {AT(fr.height), 1, TILE_OR_STEPS}, {AT(fr.disp), 2, TILE_OR_STEPS}, {AT(fr.normal), 3, TILE_OR_STEPS}, {AT(fr.white), 1, TILE_OR_STEPS},
};
#undef AT
// allocates the missing rows of `when` on the current device, or without t frees them; false: hipMalloc failed (all freed)
static bool tile_bufs_walk(mw_tiles::Local& L, int when, const mw_tiles* t) {
    for (const auto& r : tile_bufs) {
        if (!(r.when & when)) continue;
        void*& p = *reinterpret_cast<void**>(reinterpret_cast<char*>(&L) + r.at);
        if (!t) { hipFree(p); p = nullptr; continue; }
        const size_t floats = (size_t)t->N * t->N * r.floats * (r.when == TILE_OR ? 1 : t->max_steps);
        if (!p && hipMalloc(&p, sizeof(float) * floats) != hipSuccess) { tile_bufs_walk(L, when, nullptr); return false; }
    }
    return true;
}
static bool event_new(hipEvent_t* e) { return hipEventCreateWithFlags(e, hipEventDisableTiming) == hipSuccess; }
static void tiles_free_local(mw_tiles::Local& L) {
    for (int c = 0; c < 2; c++) {
        tile_bufs_walk(L, TILE_SET0 << c, nullptr);
        if (L.set[c].sent.ev) { hipEventDestroy(L.set[c].sent.ev); L.set[c].sent.ev = nullptr; }
    }
    tile_bufs_walk(L, TILE_OR | TILE_OR_STEPS, nullptr);
    if (L.done) { hipEventDestroy(L.done); L.done = nullptr; }
    if (L.ocean) { mw_ocean_destroy(L.ocean); L.ocean = nullptr; }
}

static mw_status tiles_alloc_local(mw_tiles* t, const mw_params* params, int device, int global_index) {
    mw_params p = *params;
    p.seed = params->seed + (uint64_t)global_index;
    p.device = device;
    mw_tiles::Local L;
    L.device = device; L.global_index = global_index;
    mw_status s = mw_ocean_create(&p, &L.ocean);
    if (s != MW_OK) return s;
    t->N = L.ocean->N;
    t->sem = L.ocean->sem;
    const int when = t->fm() ? TILE_SET0 : (t->max_steps > 1 ? TILE_OR | TILE_OR_STEPS : TILE_OR);
    if (!tile_bufs_walk(L, when, t) || !event_new(&L.done) || !event_new(&L.set[0].sent.ev) || !event_new(&L.set[1].sent.ev)) {
        tiles_free_local(L);
        return fail(MW_ENOMEM, "mw_tiles: output buffers of a tile could not be allocated");
    }
    t->tiles.push_back(L);
    return MW_OK;
}
// a device's side: stream and event behind a gather's sends
static bool dev_open(mw_tiles::Dev& d) {
    return hipSetDevice(d.device) == hipSuccess && hipStreamCreateWithFlags(&d.side, hipStreamNonBlocking) == hipSuccess && event_new(&d.sent.ev);
}
static mw_tiles::Local* tile_at(mw_tiles* t, int32_t k) { return (t && k >= 0 && k < (int)t->tiles.size()) ? &t->tiles[k] : nullptr; }

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
        if (d.sent.ev) hipEventDestroy(d.sent.ev);
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

typedef std::unique_ptr<mw_tiles, void (*)(mw_tiles*)> TilesGuard;  // a create form's failure exit: destroys the half-built handle AFTER fail() -- the destroy path must not fail()
mw_status mw_tiles_create(const mw_params* params, int32_t ntiles, const int32_t* devices, int32_t max_steps, mw_tiles** out) {
    DeviceGuard guard;
    mw_status s = tiles_check(params, max_steps, out);
    if (s != MW_OK) return s;
    const int ndev = mw_device_count();
    if (ndev < 1) return fail(MW_EDEVICE, "mw_tiles_create: no HIP device visible (this library has no CPU fallback)");
    if (ntiles < 1 || ntiles > 64) return fail(MW_EINVAL, "mw_tiles_create: ntiles must be in [1,64]");
    TilesGuard t(new (std::nothrow) mw_tiles(), mw_tiles_destroy);
    if (!t) return fail(MW_ENOMEM, "mw_tiles_create: out of host memory");
    t->max_steps = max_steps; t->ntiles_total = ntiles;
    for (int k = 0; k < ntiles; k++) {
        const int dev = devices ? devices[k] : k % ndev;
        if (dev < 0 || dev >= ndev) return fail(MW_EINVAL, "mw_tiles_create: bad device ordinal");
        if (!t->dev_of(dev)) { const mw_tiles::Dev d{dev, (int)t->devs.size()}; t->devs.push_back(d); }
        t->rank_of_tile.push_back(t->dev_of(dev)->rank);
        if ((s = tiles_alloc_local(t.get(), params, dev, k)) != MW_OK) return s;
    }
    for (auto& d : t->devs) if (!dev_open(d)) return fail(MW_EDEVICE, "mw_tiles_create: side stream creation failed");
    // one communicator rank per distinct device (a single device gets a 1-rank communicator: its gather is an RCCL
    // self send/receive, so the same code path runs on a 1-GPU box)
    const Rccl* R = rccl();
    if (!R) return fail(MW_EDEVICE, "RCCL is not available: " + g_rccl_err);
    std::vector<int> devlist;
    for (auto& d : t->devs) devlist.push_back(d.device);
    std::vector<mw_ncclComm_t> comms(devlist.size(), nullptr);
    int r = R->CommInitAll(comms.data(), (int)devlist.size(), devlist.data());
    if (r != MW_NCCL_SUCCESS) return fail(MW_EDEVICE, std::string("ncclCommInitAll: ") + R->GetErrorString(r));
    for (size_t i = 0; i < comms.size(); i++) t->devs[i].comm = comms[i];
    *out = t.release();
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
    TilesGuard t(new (std::nothrow) mw_tiles(), mw_tiles_destroy);
    if (!t) return fail(MW_ENOMEM, "mw_tiles_create_rank: out of host memory");
    t->max_steps = max_steps; t->ntiles_total = nranks;
    for (int k = 0; k < nranks; k++) t->rank_of_tile.push_back(k);  // tile k lives on rank k
    if ((s = tiles_alloc_local(t.get(), params, device, rank)) != MW_OK) return s;
    const mw_tiles::Dev d{device, rank};
    t->devs.push_back(d);
    if (!dev_open(t->devs.back())) return fail(MW_EDEVICE, "mw_tiles_create_rank: side stream creation failed");
    mw_ncclUniqueId id;
    std::memcpy(&id, comm_id, MW_COMM_ID_BYTES);
    int r = R->CommInitRank(&t->devs.back().comm, nranks, id, rank);
    if (r != MW_NCCL_SUCCESS) return fail(MW_EDEVICE, std::string("ncclCommInitRank: ") + R->GetErrorString(r));
    *out = t.release();
    return MW_OK;
}

int32_t mw_tiles_count(const mw_tiles* t) { return t ? t->ntiles_total : 0; }
int32_t mw_tiles_local_count(const mw_tiles* t) { return t ? (int32_t)t->tiles.size() : 0; }
mw_ocean* mw_tiles_ocean(mw_tiles* t, int32_t k) { mw_tiles::Local* L = tile_at(t, k); return L ? L->ocean : nullptr; }

mw_status mw_tiles_generate_texture_steps(mw_tiles* t, const float* delta_time, int32_t nframes) {
    if (!t || !delta_time) return fail(MW_EINVAL, "mw_tiles_generate_texture_steps: NULL argument");
    if (t->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, "mw_tiles_generate_texture_steps: OceanRenderer tiles only (FFTMesh tiles: mw_tiles_evaluate)");
    if (nframes < 1 || nframes > t->max_steps) return fail(MW_EINVAL, "mw_tiles_generate_texture_steps: nframes out of range (max_steps of mw_tiles_create)");
    DeviceGuard guard;
    for (auto& L : t->tiles) {  // asynchronous: nframes consecutive GenerateTexture() calls per tile in one enqueue, every device works at once
        mw_status s = mw_ocean_generate_texture_steps_device(L.ocean, delta_time, nframes, L.fr.height, L.fr.disp, L.fr.normal, L.fr.white);
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
    const mw_tiles::Local* L = tile_at(t, k);
    if (!L) return fail(MW_EINVAL, "mw_tiles_frames: bad tile index");
    if (t->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, "mw_tiles_frames: OceanRenderer tiles only (FFTMesh tiles: mw_tiles_outputs)");
    if (!L->fr.height) return fail(MW_ESTATE, "mw_tiles_frames: tiles created with max_steps 1 keep one frame (mw_tiles_textures)");
    store_ptrs({d_height, d_disp_xz, d_normal_xyz, d_white}, {L->fr.height, L->fr.disp, L->fr.normal, L->fr.white});
    return MW_OK;
}

mw_status mw_tiles_textures(mw_tiles* t, int32_t k, void** d_height, void** d_disp_xz, void** d_normal_xyz, void** d_white) {
    const mw_tiles::Local* L = tile_at(t, k);
    if (!L) return fail(MW_EINVAL, "mw_tiles_textures: bad tile index");
    if (t->sem != MW_SEM_OCEANRENDERER) return fail(MW_ESTATE, "mw_tiles_textures: OceanRenderer tiles only (FFTMesh tiles: mw_tiles_outputs)");
    const OrTex& s = L->ocean->orr.out;
    store_ptrs({d_height, d_disp_xz, d_normal_xyz, d_white}, {s.height, s.disp, s.normal, s.white});
    return MW_OK;
}

mw_status mw_tiles_evaluate(mw_tiles* t, const float* times, int32_t nsteps, uint32_t flags) {
    if (!t || !times) return fail(MW_EINVAL, "mw_tiles_evaluate: NULL argument");
    if (t->sem != MW_SEM_FFTMESH) return fail(MW_ESTATE, "mw_tiles_evaluate: FFTMesh tiles only (OceanRenderer tiles: mw_tiles_generate_texture)");
    if (nsteps < 1 || nsteps > t->max_steps) return fail(MW_EINVAL, "mw_tiles_evaluate: nsteps out of range");
    DeviceGuard guard;
    t->white_stride = (flags & MW_OUT_COLOR_RGBA) ? 4 : 1;
    for (auto& L : t->tiles) {  // asynchronous: one enqueue per tile, every device works at once
        mw_tiles::OutSet& set = L.set[L.next];
        if (set.sent.pending) {  // the sends of the gather that read this set (two enqueues ago) must be done before it is overwritten
            HIP_TRY(hipSetDevice(L.device));
            HIP_TRY(hipStreamWaitEvent(L.ocean->stream, set.sent.ev, 0));
            set.sent.pending = false;
        }
        mw_status s = mw_ocean_evaluate_device(L.ocean, times, nsteps, set.v, set.n, set.w, flags);
        if (s != MW_OK) return s;
        L.last = L.next;
    }
    return MW_OK;
}

mw_status mw_tiles_outputs(mw_tiles* t, int32_t k, void** d_vertices, void** d_normals, void** d_white) {
    const mw_tiles::Local* L = tile_at(t, k);
    if (!L) return fail(MW_EINVAL, "mw_tiles_outputs: bad tile index");
    if (t->sem != MW_SEM_FFTMESH) return fail(MW_ESTATE, "mw_tiles_outputs: FFTMesh tiles only (OceanRenderer tiles: mw_tiles_textures)");
    const mw_tiles::OutSet& s = L->set[L->last];  // the set the latest mw_tiles_evaluate wrote (the sets alternate once gathers are in use)
    store_ptrs({d_vertices, d_normals, d_white, nullptr}, {s.v, s.n, s.w, nullptr});
    return MW_OK;
}

// ---- the gather: every tile's finished outputs into one buffer on the root's device ----
// the root buffer, on the root's device (rootdev NULL: not in this process)
static mw_status gather_root_buffer(mw_tiles* t, const mw_tiles::Dev* rootdev) {
    if (!rootdev || (t->gathered && t->gathered_device == rootdev->device)) return MW_OK;
    if (t->gathered) { HIP_TRY(hipSetDevice(t->gathered_device)); HIP_TRY(hipFree(t->gathered)); t->gathered = nullptr; }
    HIP_TRY(hipSetDevice(rootdev->device));
    if (hipMalloc((void**)&t->gathered, sizeof(float) * (size_t)t->ntiles_total * (size_t)t->N * t->N * 10) != hipSuccess)
        return fail(MW_ENOMEM, "mw_tiles_gather: root buffer");
    t->gathered_device = rootdev->device;
    return MW_OK;
}
// FFTMesh tiles: NO copy on the compute stream.  An event behind the evaluate that wrote the set, the side stream waits for it and
// sends straight from the set; the next evaluate goes to the OTHER set (allocated here on first use) and only an evaluate that comes
// back to this set -- two enqueues later -- waits for these sends.  OceanRenderer tiles (one frame per call, textures inside the
// handle) keep the snapshot: a 28-MB device copy per frame, then the send of the snapshot.
static mw_status gather_ready(mw_tiles* t, int step) {
    for (auto& L : t->tiles) {
        HIP_TRY(hipSetDevice(L.device));
        mw_tiles::Dev* d = t->dev_of(L.device);
        hipStream_t cs = L.ocean->stream;
        if (t->fm() && !tile_bufs_walk(L, TILE_SET0 << (L.last ^ 1), t)) {
            (void)hipGetLastError();
            return fail(MW_ENOMEM, "mw_tiles_gather: second output set of a tile could not be allocated");
        }
        if (!t->fm()) {
            if (d->sent.pending) HIP_TRY(hipStreamWaitEvent(cs, d->sent.ev, 0));
            for (int a = 0; a < t->nparts(); a++)
                HIP_TRY(hipMemcpyAsync(L.staged + t->part_offset(a), t->part_src(L, a, step), t->part_count(a) * sizeof(float), hipMemcpyDeviceToDevice, cs));
        }
        HIP_TRY(hipEventRecord(L.done, cs));
        HIP_TRY(hipStreamWaitEvent(d->side, L.done, 0));
    }
    return MW_OK;
}
// Tiles that already live on the root's device do not travel: their step is copied into the root buffer on that device's side
// stream (device-local, no communicator: round 4 sent them to themselves through RCCL, whose copy kernel held CUs for the length of
// a 29-MB transfer -- on one device the gather cost 11 % of the step rate, 7 % once the snapshot was gone; profiles/r05_ab_notes.md).
// RCCL carries what crosses devices, which is what it is for.
static mw_status gather_home_copies(mw_tiles* t, const mw_tiles::Dev* home, int step) {
    // (a blit kernel: the SDMA engines -- hipMemcpyDeviceToDeviceNoCU -- measured slower, with-gather 0.858 of without against 0.948)
    const hipMemcpyKind home_kind = hipMemcpyDeviceToDevice;
    for (auto& L : t->tiles) {
        if (!home || L.device != home->device) continue;
        HIP_TRY(hipSetDevice(L.device));
        float* dst = t->gathered + (size_t)L.global_index * t->floats_per_tile();
        for (int a = 0; a < t->nparts(); a++)
            HIP_TRY(hipMemcpyAsync(dst + t->part_offset(a), t->send_src(L, a, step), t->part_count(a) * sizeof(float), home_kind, home->side));
    }
    return MW_OK;
}
// the one RCCL group's calls: they stop at the first error, made by the call *what names
static int gather_sends_recvs(mw_tiles* t, const Rccl* R, const mw_tiles::Dev* rootdev, const mw_tiles::Dev* home, int root_rank, int step,
                              const char** what) {
    const int np = t->nparts();
    int err = MW_NCCL_SUCCESS;
    *what = "ncclSend";
    for (auto& L : t->tiles) {  // sends of the local tiles that cross devices (the parts of each in a fixed order)
        if (home && L.device == home->device) continue;
        mw_tiles::Dev* d = t->dev_of(L.device);
        for (int a = 0; a < np && err == MW_NCCL_SUCCESS; a++)
            err = R->Send(t->send_src(L, a, step), t->part_count(a), MW_NCCL_FLOAT32, root_rank, d->comm, d->side);
    }
    if (!rootdev || err != MW_NCCL_SUCCESS) return err;
    *what = "ncclRecv";
    for (int k = 0; k < t->ntiles_total && err == MW_NCCL_SUCCESS; k++) {  // receives on the root: tiles in global order; tiles of one rank arrive in that rank's send order
        if (home && t->rank_of_tile[k] == root_rank) continue;  // a tile of the root's own rank = of the root's device: copied already
        float* dst = t->gathered + (size_t)k * t->floats_per_tile();
        for (int a = 0; a < np && err == MW_NCCL_SUCCESS; a++)
            err = R->Recv(dst + t->part_offset(a), t->part_count(a), MW_NCCL_FLOAT32, t->rank_of_tile[k], rootdev->comm, rootdev->side);
    }
    return err;
}
// an event that cannot be recorded: wait for the stream instead
static void record_or_wait(int device, mw_tiles::Sent& sent, hipStream_t side) {
    if (hipSetDevice(device) == hipSuccess && hipEventRecord(sent.ev, side) == hipSuccess) { sent.pending = true; return; }
    (void)hipGetLastError();
    (void)hipStreamSynchronize(side);
}
// Sends and home copies may already sit on the side streams whatever RCCL returned, and the set they read must not be handed to the
// next evaluate before they are done.
static void gather_bookkeeping(mw_tiles* t) {
    for (auto& d : t->devs) record_or_wait(d.device, d.sent, d.side);
    if (!t->fm()) return;
    for (auto& L : t->tiles) {  // the set just sent is busy until its sends are done; the next evaluate writes the other one
        record_or_wait(L.device, L.set[L.last].sent, t->dev_of(L.device)->side);
        L.next = L.last ^ 1;
    }
}

mw_status mw_tiles_gather(mw_tiles* t, int32_t step, int32_t root) {
    if (!t) return fail(MW_EINVAL, "NULL handle");
    if (step < 0 || step >= t->max_steps || root < 0 || root >= t->ntiles_total) return fail(MW_EINVAL, "mw_tiles_gather: bad step / root");
    if (t->sem == MW_SEM_OCEANRENDERER)
        for (auto& L : t->tiles)
            if (L.fr.height && step >= L.frames) return fail(MW_EINVAL, "mw_tiles_gather: the latest mw_tiles_generate_texture_steps wrote fewer frames than `step`");
    const Rccl* R = rccl();
    if (!R) return fail(MW_EDEVICE, "RCCL is not available: " + g_rccl_err);
    if (t->sem == MW_SEM_OCEANRENDERER)
        for (auto& L : t->tiles)
            if (!L.ocean->orr.have_frame) return fail(MW_ESTATE, "mw_tiles_gather: no GenerateTexture() yet");
    DeviceGuard guard;
    const int root_rank = t->rank_of_tile[root];
    mw_tiles::Dev* rootdev = nullptr;
    for (auto& d : t->devs) if (d.rank == root_rank) rootdev = &d;
    // (switch MW_TILES_FORCE_RCCL = 1: every tile goes through ncclSend / ncclRecv, the root's own included -- how the GPU tests keep
    // the communicator path exercised on a 1-GPU box)
    const mw_tiles::Dev* home = sw(SW_TILES_FORCE_RCCL) != 0 ? nullptr : rootdev;  // its tiles do not travel
    mw_status s;
    if ((s = gather_root_buffer(t, rootdev)) != MW_OK || (s = gather_ready(t, step)) != MW_OK || (s = gather_home_copies(t, home, step)) != MW_OK) return s;
    // One RCCL group.  A failing Send / Recv must not leave the thread's group open (every later RCCL call of this thread --
    // torch's included -- would queue behind it for ever): remember the first error, always end the group, then report.  Bookkeeping first.
    const char* first_what = nullptr;
    RCCL_TRY(R, R->GroupStart());
    const int first_err = gather_sends_recvs(t, R, rootdev, home, root_rank, step, &first_what);
    const int end_err = R->GroupEnd();
    gather_bookkeeping(t);
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
