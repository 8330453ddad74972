"""Helpers of tests/test_pond_sizes_gpu.py: guarded output buffers, the pond's stated bounds, the three kernels behind one call shape,
and the float64 oracle walked in slices.

Guards.  guarded(nfloats, lead) is ONE buffer of nfloats + 2 * 64 + lead floats filled, through an int32 view, with a quiet-NaN bit
pattern that no finite result can equal; the payload starts 64 + lead floats in (lead = 0 keeps the allocation's 16-byte alignment,
1 or 3 breaks it).  A store past either end of the payload changes a guard word (assert_guards_intact compares both regions bit for
bit), a vertex that was never stored keeps the pattern (assert_all_written).

Bounds.  The project's own, stated where they were first used (tests/test_gpu_parity.py): B_SINGLE for mw_gerstner_displace* with the 8
pond waves on coordinates in [-50, 50], B_STEPS for the steps entry and B_POND for PondMaterial positions and normals on
workloads.pond_lattice's range, bound(wv, t) for any other wave set.

Reference.  oracle.gerstner_f64 / oracle.pond_displace_f64 over windows of at most 2^20 vertices, at most four windows' float64 arrays
alive at a time (tests/memguard.py says why that matters)."""
import ctypes as C

import numpy as np

import workloads

P = workloads.POND
M = workloads.POND_MATERIAL
GUARD = 64                  # floats on either side of a payload
SENTINEL = 0x7FC5A5A5       # a quiet NaN with a payload of its own: never the result of arithmetic on finite inputs
CHUNK = 1 << 20             # vertices per oracle call
B_SINGLE = 2e-5 + 8e-6      # test_gerstner_pond
B_STEPS = 8e-6              # test_gerstner_time_batched
B_POND = 6e-6               # test_pond_material_displacement_modes


def bound(wv, t):
    # the shader's phase theta = frequency * dot(dir, x) + t * speed is FLOAT32 (W/MistralWaterLib.cginc:80-84, `half` = f32 on desktop),
    # the oracle's f64: each of theta's roundings (the product t * speed, the sum) moves it by up to half an ulp of |theta|, and an
    # offset moves by at most its amplitude times that, per wave
    wv = np.asarray(wv, np.float64).reshape(-1, 3)
    th = np.abs(P["frequency"] * (wv[:, 0] * 50.0 * 1.0 + np.abs(wv[:, 1]) * 50.0)) + abs(t) * np.abs(wv[:, 2])
    ulp = float(np.spacing(np.float32(th.max())))
    return 2e-5 + 8e-6 + len(wv) * max(P["amplitude"], P["amplitude"] * P["steepness"]) * 1.5 * ulp


def waves16():
    """The 8 pond waves, then the same 8 rotated by 45 degrees at 0.75 x the speed."""
    w = list(workloads.pond_waves8())
    c = s = float(np.sqrt(0.5))
    return w + [(c * dx - s * dy, s * dx + c * dy, 0.75 * sp) for (dx, dy, sp) in w]


def positions(nv, seed):
    """nv vertices with x, z uniform in [-50, 50) and y within pond_lattice's jitter of 0.25: inside the range of every stated bound."""
    rng = np.random.default_rng(seed)
    pos = rng.uniform(-50.0, 50.0, (nv, 3)).astype(np.float32)
    pos[:, 1] = (0.25 + rng.uniform(-0.04, 0.04, nv)).astype(np.float32)
    return pos


# ---- guarded buffers ---------------------------------------------------------------------------------------------------------------
def _is_np(x):
    return isinstance(x, np.ndarray)


def _words(x):
    if _is_np(x):
        return x.view(np.int32)
    import torch
    return x.view(torch.int32)


class Guarded:
    """buf: the whole buffer; payload: its nfloats floats between the guards; ptr: the payload's address."""

    def __init__(self, buf, nfloats, lead):
        self.buf, self.nfloats, self.lead = buf, int(nfloats), int(lead)
        self.payload = buf[GUARD + lead:GUARD + lead + nfloats]
        self.ptr = self.payload.ctypes.data if _is_np(buf) else self.payload.data_ptr()
        assert (self.ptr % 16 == 0) == (lead % 4 == 0), (self.ptr, lead)


def guarded(nfloats, lead=0, host=False):
    """A sentinel-filled buffer with its payload 64 + lead floats in: on the device (torch), or host=True in host memory (numpy)."""
    n = int(nfloats) + 2 * GUARD + int(lead)
    if host:
        buf = np.empty(n, np.float32)
        buf.view(np.int32)[:] = SENTINEL
    else:
        import torch
        buf = torch.empty(n, dtype=torch.float32, device="cuda")
        buf.view(torch.int32).fill_(SENTINEL)
    return Guarded(buf, nfloats, lead)


def assert_guards_intact(g, tag=""):
    lo, hi = _words(g.buf[:GUARD + g.lead]), _words(g.buf[GUARD + g.lead + g.nfloats:])
    assert len(lo) == GUARD + g.lead and len(hi) == GUARD
    for name, w in (("front", lo), ("back", hi)):
        bad = (w != SENTINEL).nonzero()
        bad = bad[0] if _is_np(w) else bad[:, 0].cpu().numpy()
        assert len(bad) == 0, f"{tag}: {len(bad)} words of the {name} guard were overwritten, first at guard word {int(bad[0])}"


def assert_all_written(payload, tag=""):
    w = _words(payload.reshape(-1))
    step = 1 << 27                                   # (a comparison's boolean temporary stays at 128 MB)
    for a in range(0, len(w), step):
        miss = w[a:a + step] == SENTINEL
        if bool(miss.any()):
            idx = miss.nonzero()
            first = int(idx[0][0]) if _is_np(w) else int(idx[0, 0])
            raise AssertionError(f"{tag}: {int(miss.sum())} words in [{a}, {a + step}) were never written, first at float {a + first} "
                                 f"(vertex {(a + first) // 3} of a [.., nverts, 3] slab run)")


def assert_untouched(g, tag=""):
    """a refused call left the whole buffer, payload included, as it was"""
    w = _words(g.buf)
    assert bool((w == SENTINEL).all()), f"{tag}: the buffer of a refused call was written"


def assert_bits_equal(a, b, tag=""):
    """a and b (torch device tensors or numpy arrays, any mix, any strides) hold the same words"""
    if _is_np(a) or _is_np(b):
        a = a if _is_np(a) else a.cpu().numpy()
        b = b if _is_np(b) else b.cpu().numpy()
    a, b = _words(a), _words(b)
    assert a.shape == b.shape, (tag, tuple(a.shape), tuple(b.shape))
    if _is_np(a):
        ne = a != b
        assert not ne.any(), f"{tag}: {int(ne.sum())} words differ, first at {tuple(int(i[0]) for i in ne.nonzero())}"
        return
    if a.dim() > 1:                                  # slab by slab: a comparison's boolean temporary stays small
        for r in range(a.shape[0]):
            assert_bits_equal(a[r], b[r], f"{tag}[{r}]")
        return
    step = 1 << 27
    for r in range(0, a.shape[0], step):
        ne = a[r:r + step] != b[r:r + step]
        if bool(ne.any()):
            raise AssertionError(f"{tag}: {int(ne.sum())} words differ in [{r}, {r + step}), first at float {r + int(ne.nonzero()[0, 0])}")


# ---- the three kernels behind one call shape ---------------------------------------------------------------------------------------
def _vp(p):
    return C.c_void_p(int(p)) if p else None


def _stream():
    import torch
    return _vp(torch.cuda.current_stream().cuda_stream)


class Op:
    """One entry point with its parameters fixed.  run(mw, d_pos, nv, ptrs) launches it on torch's current stream and returns the
    status; it writes `nouts` buffers of K * nv * 3 floats ([K][nv][3]).  ref(oracle, pos, k) is the float64 reference of slab k on
    host positions pos [n, 3], one array per output; tol the stated bound.  host(mw, pos_ptr, nv, ptrs): the host form, where there
    is one."""

    def __init__(self, name, nouts, K, run, ref, tol, host=None):
        self.name, self.nouts, self.K, self.run, self.ref, self.tol, self.host = name, nouts, K, run, ref, tol, host

    def __repr__(self):
        return self.name


def gerstner_op(waves, t, nwaves=None):
    """mw_gerstner_displace_device (k_gerstner); nwaves overrides the count that is passed (the refused counts)."""
    wv = np.ascontiguousarray(waves, np.float32).reshape(-1, 3)
    nw = wv.shape[0] if nwaves is None else nwaves
    a = (C.c_float(P["amplitude"]), C.c_float(P["frequency"]), C.c_float(P["steepness"]), C.c_float(t))

    def run(mw, d_pos, nv, ptrs):
        return mw.lib().mw_gerstner_displace_device(_vp(d_pos), nv, wv.ctypes.data_as(C.c_void_p), nw, *a, _vp(ptrs[0]), _stream())

    def host(mw, pos_ptr, nv, ptrs):
        return mw.lib().mw_gerstner_displace(_vp(pos_ptr), nv, wv.ctypes.data_as(C.c_void_p), nw, *a, _vp(ptrs[0]), 0)

    def ref(oracle, pos, k):
        return (oracle.gerstner_f64(pos, wv, P["amplitude"], P["frequency"], P["steepness"], np.float32(t)),)

    pond8 = nw == 8 and np.array_equal(wv, np.asarray(workloads.pond_waves8(), np.float32))
    return Op(f"gerstner{nw}", 1, 1, run, ref, B_SINGLE if pond8 and t == 3.25 else bound(wv, t), host)


def steps_op(nw, times, nwaves=None):
    """mw_gerstner_displace_steps_device (k_gerstner_steps<4|8>) with the first nw pond waves and these time values."""
    wv = np.ascontiguousarray(waves16()[:nw], np.float32).reshape(-1, 3)
    tt = np.ascontiguousarray(times, np.float32)
    a = (C.c_float(P["amplitude"]), C.c_float(P["frequency"]), C.c_float(P["steepness"]))

    def run(mw, d_pos, nv, ptrs):
        return mw.lib().mw_gerstner_displace_steps_device(_vp(d_pos), nv, wv.ctypes.data_as(C.c_void_p), nw if nwaves is None else nwaves,
                                                          *a, tt.ctypes.data_as(C.c_void_p), tt.size, _vp(ptrs[0]), _stream())

    def ref(oracle, pos, k):
        return (oracle.gerstner_f64(pos, wv, P["amplitude"], P["frequency"], P["steepness"], tt[k]),)

    return Op(f"steps{nw}x{tt.size}", 1, int(tt.size), run, ref, B_STEPS)


def pond_op(mw, oracle, mode, normals, t=3.25):
    """mw_pond_displace_device (k_pond<normals>) on the shipped material; GerstnerLevelOne at the amplitude its bound was stated for."""
    amp = 0.1 if mode == mw.MW_POND_GERSTNER_LEVEL_ONE else M["_Amplitude"]
    mat = mw.PondMaterial(mode=mode, **{**M, "_Amplitude": amp})
    op = oracle.pond_params(mode, amplitude=amp, frequency=M["_Frequency"], speed=M["_Speed"], steepness=M["_Steepness"],
                            smoothing=M["_Smoothing"], wspeed=M["_WSpeed"], dir_ab=M["_WDirectionAB"], dir_cd=M["_WDirectionCD"])

    def run(mw_, d_pos, nv, ptrs):
        p = mat._c()
        return mw_.lib().mw_pond_displace_device(C.byref(p), _vp(d_pos), nv, C.c_float(t), _vp(ptrs[0]), _vp(ptrs[1]) if normals else None,
                                                 _stream())

    def host(mw_, pos_ptr, nv, ptrs):
        p = mat._c()
        return mw_.lib().mw_pond_displace(C.byref(p), _vp(pos_ptr), nv, C.c_float(t), _vp(ptrs[0]), _vp(ptrs[1]) if normals else None, 0)

    def ref(oracle_, pos, k):
        return oracle_.pond_displace_f64(op, pos, t)[:2 if normals else 1]

    return Op(f"pond{mode}{'n' if normals else ''}", 2 if normals else 1, 1, run, ref, B_POND, host)


# ---- the float64 reference in windows ----------------------------------------------------------------------------------------------
def chunks(nv):
    """every vertex, in windows of at most 2^20"""
    return [(a, min(a + CHUNK, nv)) for a in range(0, nv, CHUNK)]


def edges(nv, w=4096):
    """the first and the last w vertices of every 2^20-vertex slice"""
    out = []
    for a, b in chunks(nv):
        out += [(a, b)] if b - a <= 2 * w else [(a, a + w), (b - w, b)]
    return out


def oracle_errors(oracle, op, pos, outs, nv, windows, steps=None):
    """max |device - float64| per output of `op` over the windows [(a, b), ...] of the slabs `steps` (default: all); pos: the
    positions [nv, 3] (a host array, or a device tensor whose windows are copied), outs: the Guarded device outputs.  One window of one
    slab is on the host per worker: the oracle is one C loop that releases the interpreter lock, so four windows run side by side (at
    most 4 x 2^20 vertices of float64 results, ~150 MB)."""
    from concurrent.futures import ThreadPoolExecutor

    def window(kab):
        k, a, b = kab
        assert 0 <= a < b <= nv and b - a <= CHUNK
        p = pos[a:b] if _is_np(pos) else pos[a:b].cpu().numpy()
        want = op.ref(oracle, p, k)
        err = []
        for i in range(op.nouts):
            got = outs[i].payload.view(op.K, nv, 3)[k, a:b].cpu().numpy()
            assert np.isfinite(got).all(), (op, i, k, a, b)
            err.append(float(np.abs(got - want[i]).max()))
        return err

    tasks = [(k, a, b) for k in (range(op.K) if steps is None else steps) for a, b in windows]
    if len(tasks) < 4:
        errs = [window(t) for t in tasks]
    else:
        with ThreadPoolExecutor(4) as ex:
            errs = list(ex.map(window, tasks))
    return [max(e[i] for e in errs) for i in range(op.nouts)]
