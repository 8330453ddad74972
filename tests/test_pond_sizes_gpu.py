"""GPU tier of the pond kernels' index work (k_gerstner, k_gerstner_steps<4|8>, k_pond<NORMALS>) through the C ABI: the grid-stride trips
behind the 4096-workgroup launch cap, wave_store_3f4's LDS turn and its nf4 tail mask, the float4 body / scalar tail / alignment decision,
the (vertex block, step group) grid with its step_hi clamp, and slab offsets past 2^31 elements and 2^32 bytes.  The per-vertex
arithmetic is held elsewhere (tests/test_emul.py, tests/test_gpu_parity.py); here every call writes into sentinel-filled buffers between
guard words (tests/pond_ref.py), every output is checked for words that were never stored, and results are held two ways:

  * against the float64 oracle under the bounds the project already states (pond_ref.B_SINGLE / B_STEPS / B_POND, bound());
  * bit for bit, on the device, against calls of the same entry point that stay below the cap: consecutive slices of the same input
    whose starts are multiples of 1024 vertices.  A vertex's lane and unrolled slot depend on its index modulo 256 in all three
    kernels (float4 kernels: lane = quad index mod 64, slot = index mod 4; steps kernel: k * 64 + lane within a 256-vertex chunk), so
    it runs the same instructions in both calls: equal bits are a property of the index maps, not of the compiler.

The cap bites above 4 * 2^20 vertices (float4 path: 4 per thread; steps kernel: 1024 per workgroup) and above 2^20 on the scalar path
that unaligned buffers take."""
import numpy as np
import pytest

import pond_ref as R

pytestmark = pytest.mark.gpu
CAP = 4 << 20                                      # vertices one launch serves without a second grid-stride trip
T = 3.25
NV_BIG = 2 * CAP + 261                             # two full trips, then a partial wave (65 quads) and one scalar tail vertex
NV_UNALIGNED = (2 << 20) + 7                       # the scalar path's third trip
SIZES = (1, 2, 3, 4, 5, 7, 8, 252, 255, 256, 257, 260, 1020, 1023, 1024, 1025, 1028, 65535, 65536, 65537)
TIMES32 = [0.0, -7.5, 600.0] + [(k + 1) / 60.0 for k in range(3, 32)]      # distinct; the first K of them are a call's time values
OPS = ("gerstner8", "pond_wave_n", "pond_gerstner_n", "pond_level_one_n", "pond_wave", "steps8x3", "steps4x9")
_cache = {}


def op_of(mw, oracle, name):
    if name == "gerstner8":
        return R.gerstner_op(R.waves16()[:8], T)
    if name.startswith("steps"):
        nw, K = (int(x) for x in name[5:].split("x"))
        return R.steps_op(nw, TIMES32[:K])
    mode = {"wave": mw.MW_POND_WAVE, "gerstner": mw.MW_POND_GERSTNER, "level_one": mw.MW_POND_GERSTNER_LEVEL_ONE}
    normals = name.endswith("_n")
    return R.pond_op(mw, oracle, mode[name[5:-2] if normals else name[5:]], normals, T)


@pytest.fixture(scope="module", autouse=True)
def _release():
    """the host positions and torch's cached device blocks go back when the file is done"""
    yield
    _cache.clear()
    import torch
    torch.cuda.empty_cache()


def inputs(nv, seed):
    """host positions [nv, 3] (made once per size and seed, never written) and device(lead): a copy of them in a guarded device buffer"""
    import torch
    if ("pos", nv, seed) not in _cache:
        _cache["pos", nv, seed] = R.positions(nv, seed)
    pos = _cache["pos", nv, seed]

    def device(lead=0):
        g = R.guarded(nv * 3, lead)
        g.payload.copy_(torch.from_numpy(pos).reshape(-1))
        return g
    return pos, device


def run(mw, op, d_pos, nv, leads=(0, 0), tag=""):
    """one call of `op` into fresh guarded buffers (leads: one per output); guards and all-written are asserted"""
    outs = [R.guarded(op.K * nv * 3, leads[i]) for i in range(op.nouts)]
    assert op.run(mw, d_pos, nv, [o.ptr for o in outs]) == mw.MW_OK, (op, tag, mw.lib().mw_last_error())
    for i, o in enumerate(outs):
        R.assert_guards_intact(o, f"{op} {tag} output {i}")
        R.assert_all_written(o.payload, f"{op} {tag} output {i}")
    return outs


def slab(o, op, nv):
    """[K][nv * 3] view of an output"""
    return o.payload.view(op.K, nv * 3)


def assert_slice_rule(mw, op, d_pos, nv, outs, size=CAP):
    """the large call equals, bit for bit, calls below the cap on consecutive slices of the same input (starts multiples of 1024)"""
    assert size % 1024 == 0 and size <= CAP
    for a in range(0, nv, size):
        n = min(size, nv - a)
        part = run(mw, op, d_pos + 12 * a, n, tag=f"slice at {a}")
        for i in range(op.nouts):
            R.assert_bits_equal(slab(outs[i], op, nv)[:, 3 * a:3 * (a + n)], slab(part[i], op, n), f"{op} output {i}, slice at vertex {a}")
        del part


def assert_oracle(oracle, op, pos, outs, nv, windows, steps=None, tol=None):
    err = R.oracle_errors(oracle, op, pos, outs, nv, windows, steps)
    tol = op.tol if tol is None else tol
    print(f"{op} nv={nv}: max |device - f64| = {['%.3g' % e for e in err]} (bound {tol:.3g})")
    assert max(err) < tol, (op, nv, err, tol)


# ---- 1. past the launch cap, aligned -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OPS)
def test_past_the_launch_cap_aligned(mw, oracle, name):
    """8 * 2^20 + 261 vertices: two full grid-stride trips, then a third of 65 quads in one partial wave plus a scalar tail vertex (float4
    kernels), or of one workgroup with a 5-vertex chunk (steps kernel; 4 waves x 9 steps cross the cap with a last step group of one).
    Float64 oracle at every vertex of every slab, slice rule, guards, all-written."""
    op = op_of(mw, oracle, name)
    nv = NV_BIG
    pos, device = inputs(nv, 11)
    dp = device()
    outs = run(mw, op, dp.ptr, nv)
    assert_slice_rule(mw, op, dp.ptr, nv, outs)
    assert_oracle(oracle, op, pos, outs, nv, R.chunks(nv))


# ---- 2. past the scalar path's cap, unaligned ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", OPS)
def test_past_the_scalar_cap_unaligned(mw, oracle, name):
    """Buffers 4 and 12 bytes off a 16-byte boundary, both or one of them (for k_pond<true> also the normal buffer alone): the float4
    path must not be taken, the scalar loop makes its third trip at 2 * 2^20 + 7 vertices, and the result equals the aligned call's
    bit for bit.  The steps kernel has no alignment requirement; it runs unaligned above its cap."""
    op = op_of(mw, oracle, name)
    nv = CAP + 7 if op.K > 1 else NV_UNALIGNED
    pos, device = inputs(nv, 12)
    dp = device()
    want = run(mw, op, dp.ptr, nv, tag="aligned")
    assert_oracle(oracle, op, pos, want, nv, R.edges(nv))
    leads = [(1, 1, 1), (3, 3, 3), (0, 1, 1), (1, 0, 0)] + ([(0, 0, 1)] if op.nouts == 2 else [])
    for lp, lo, ln in leads:
        dq = dp if lp == 0 else device(lp)
        got = run(mw, op, dq.ptr, nv, leads=(lo, ln), tag=f"leads {lp, lo, ln}")
        assert dq.ptr % 16 == 4 * lp and got[0].ptr % 16 == 4 * lo
        for i in range(op.nouts):
            R.assert_bits_equal(got[i].payload, want[i].payload, f"{op} leads {lp, lo, ln} output {i}")
        del got


# ---- 3. wave, quad and workgroup tails -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nv", SIZES)
def test_wave_quad_and_workgroup_tails(mw, oracle, nv):
    """nf4 from 3 to 192 in the last wave, 0 / 1 / 63 / 64 / 65 quads, a scalar tail of 0 to 3 vertices behind a vector body, and for the
    steps kernel ok[k] false in 0 to 3 of a lane's four slots: float64 oracle at every vertex, guards, all-written."""
    pos, _ = inputs(SIZES[-1], 13)
    pos = pos[:nv]
    import torch
    dp = R.guarded(nv * 3)
    dp.payload.copy_(torch.from_numpy(pos).reshape(-1))
    for name in ("gerstner8", "pond_wave_n", "pond_wave", "steps8x2"):
        op = op_of(mw, oracle, name)
        outs = run(mw, op, dp.ptr, nv)
        assert_oracle(oracle, op, pos, outs, nv, R.chunks(nv))


# ---- 4. every step count ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nw", (4, 8))
def test_every_step_count(mw, oracle, nw):
    """K = 1..32 time values in one call (step groups of 8: full, unfilled, single): EVERY step k equals the K = 1 call at t[k] bit for bit
    (the launcher forms cb / sb per step from t[k] alone); float64 oracle at every step for K in {1, 8, 9, 17, 31, 32}."""
    nv = 1003
    pos, device = inputs(nv, 14)
    dp = device()
    single = [run(mw, R.steps_op(nw, [t]), dp.ptr, nv, tag=f"t = {t}")[0] for t in TIMES32]
    for K in range(1, 33):
        op = R.steps_op(nw, TIMES32[:K])
        out = run(mw, op, dp.ptr, nv)
        for k in range(K):
            R.assert_bits_equal(slab(out[0], op, nv)[k], single[k].payload, f"{op} step {k}")
        if K in (1, 8, 9, 17, 31, 32):
            assert_oracle(oracle, op, pos, out, nv, R.chunks(nv))


def test_refused_step_and_wave_counts_write_nothing(mw):
    """33 steps, and 1, 5 or 16 waves on the steps entry, are MW_EINVAL and leave the output buffer as it was."""
    nv = 1003
    _, device = inputs(nv, 14)
    dp = device()
    for op in [R.steps_op(8, [0.1 * k for k in range(33)])] + [R.steps_op(8, TIMES32[:3], nwaves=n) for n in (1, 5, 16)]:
        g = R.guarded(33 * nv * 3)
        assert op.run(mw, dp.ptr, nv, [g.ptr]) == mw.MW_EINVAL, op
        R.assert_untouched(g, str(op))


# ---- 5. every wave count of the single-step kernel -----------------------------------------------------------------------------
def test_every_wave_count(mw, oracle):
    """1..16 waves (the 8 pond waves, then the same 8 rotated by 45 degrees at 0.75 x the speed) on 4099 vertices in [-50, 50]^3, under
    bound(wv, t); 0 and 17 waves are MW_EINVAL and write nothing."""
    import torch
    nv = 4099
    pos = np.random.default_rng(15).uniform(-50, 50, (nv, 3)).astype(np.float32)
    dp = R.guarded(nv * 3)
    dp.payload.copy_(torch.from_numpy(pos).reshape(-1))
    W = R.waves16() + [(1.0, 0.0, 1.0)]
    for t in (T, -7.5):
        for nw in range(1, 17):
            op = R.gerstner_op(W[:nw], t)
            outs = run(mw, op, dp.ptr, nv)
            assert_oracle(oracle, op, pos, outs, nv, R.chunks(nv), tol=R.bound(W[:nw], t))
    for nw, wv in ((0, W[:16]), (17, W)):
        g = R.guarded(nv * 3)
        assert R.gerstner_op(wv, T, nwaves=nw).run(mw, dp.ptr, nv, [g.ptr]) == mw.MW_EINVAL, nw
        R.assert_untouched(g, f"{nw} waves")


# ---- 6. offsets past 2^31 elements and 2^32 bytes ------------------------------------------------------------------------------
def _needs_24gb():
    import torch
    free = torch.cuda.mem_get_info()[0]
    if free < 24 * 2 ** 30:
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free; this test allocates up to 15 GB and asks for 24 GiB")


def _device_positions(nv, seed):
    """x, z uniform in [-50, 50], y within pond_lattice's jitter of 0.25, generated on the device with a seeded generator"""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    pos = torch.empty(nv * 3, dtype=torch.float32, device="cuda")
    pos.uniform_(-50.0, 50.0, generator=g)
    pos.view(nv, 3)[:, 1].mul_(0.0008).add_(0.25)
    return pos


def test_steps_slabs_past_2_31_elements(mw, oracle):
    """4 waves x 32 steps on 23 * 2^20 + 5 vertices: 2.3 G floats (9.3 GB) of output, slab offsets pass 2^31 elements at step 30.  Every slab
    equals the K = 1 call at its time bit for bit (compared on the device); float64 oracle on the first and last 4096 vertices of steps 0,
    29, 30 and 31."""
    import torch
    _needs_24gb()
    nv, K = 23 * (1 << 20) + 5, 32
    times = TIMES32
    assert 29 * nv * 3 < 2 ** 31 < 30 * nv * 3
    try:
        d_pos = _device_positions(nv, 16)
        op = R.steps_op(4, times)
        outs = run(mw, op, d_pos.data_ptr(), nv)
        for k in range(K):
            one = run(mw, R.steps_op(4, [times[k]]), d_pos.data_ptr(), nv, tag=f"K = 1 at step {k}")
            R.assert_bits_equal(slab(outs[0], op, nv)[k], one[0].payload, f"{op} slab {k}")
            del one
        assert_oracle(oracle, op, d_pos.view(nv, 3), outs, nv, [(0, 4096), (nv - 4096, nv)], steps=(0, 29, 30, 31))
    finally:
        d_pos = outs = one = None
        torch.cuda.empty_cache()


@pytest.mark.parametrize("name", ("gerstner8", "pond_gerstner_n"))
def test_arrays_past_2_32_bytes(mw, oracle, name):
    """2^28 + 2^27 + 5 vertices: each array is 4.8 GB, byte offsets pass 2^32 (and float offsets 2^30).  Slice rule over the whole array in
    slices of 4 * 2^20 vertices; float64 oracle on 4096 vertices at the start, at the end, across the last slice boundary and around the
    vertices whose byte offsets are nearest 2^31 and 2^32; guards, all-written."""
    import torch
    _needs_24gb()
    nv = (1 << 28) + (1 << 27) + 5
    try:
        op = op_of(mw, oracle, name)
        d_pos = _device_positions(nv, 17)
        outs = run(mw, op, d_pos.data_ptr(), nv)
        assert_slice_rule(mw, op, d_pos.data_ptr(), nv, outs)
        last = nv // CAP * CAP
        mids = [last, 2 ** 31 // 12, 2 ** 32 // 12]
        assert_oracle(oracle, op, d_pos.view(nv, 3), outs, nv, [(0, 4096), (nv - 4096, nv)] + [(m - 2048, min(m + 2048, nv)) for m in mids])
    finally:
        d_pos = outs = None
        torch.cuda.empty_cache()


# ---- 7. host forms at a cap-crossing size --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("gerstner8", "pond_wave_n", "pond_wave"))
def test_host_forms_past_the_cap(mw, oracle, name):
    """mw_gerstner_displace and mw_pond_displace (with and without normals) at 4 * 2^20 + 5 vertices equal the device forms on the same
    input bit for bit: the two or three 256-byte-aligned staging regions at a size where the grid-stride trip runs."""
    op = op_of(mw, oracle, name)
    nv = CAP + 5
    pos, device = inputs(nv, 18)
    dp = device()
    want = run(mw, op, dp.ptr, nv)
    assert_oracle(oracle, op, pos, want, nv, R.edges(nv))
    got = [R.guarded(nv * 3, host=True) for _ in range(op.nouts)]
    assert op.host(mw, pos.ctypes.data, nv, [g.ptr for g in got]) == mw.MW_OK, mw.lib().mw_last_error()
    for i in range(op.nouts):
        R.assert_guards_intact(got[i], f"{op} host output {i}")
        R.assert_all_written(got[i].payload, f"{op} host output {i}")
        R.assert_bits_equal(got[i].payload, want[i].payload, f"{op} host form output {i}")
