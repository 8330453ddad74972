"""GPU tier: the batched FFTMesh enqueue (mw_ocean_evaluate_device with up to 32 time-steps: one launch of k_pass1, one of k_pass2 /
k_pass2_hs -- the path bench.py times) at EVERY batch size 1 .. 32 and EVERY step of it, at every FFT grid size.

FFTMesh is a pure function of (h0, h0conj, t), so step k of a batch must be, bit for bit, the frame the same time gives when it is
enqueued alone (the frame plan's kernels at 256^2 .. 1024^2, the batched kernels with nsteps = 1 elsewhere); the arithmetic of that
frame rests on the float64 oracle gates of tests/test_gpu_parity.py, and on two interior steps held to the oracle here.  What is held:

  * both grids of pass 1 at every size: the 1-D p1_block_map grid with its padding blocks (time groups of 2 .. 8) and the plain
    (GX, nsteps) grid (nsteps = 1, 11, 13, 17, 19, 23, 29, 31); the test states which one ran (mw_debug_pass1_time_group against
    the rule of tests/p1_groups.py);
  * the switch MW_P1_TGROUP: any cap gives the same frames;
  * what an enqueue leaves alone: output buffers are filled with the all-ones bit pattern (a NaN) first, the slots behind the last
    step asked for and a guard slot on either side of the buffer must still hold it;
  * enqueues of different sizes back to back on one handle with no host wait between them (growth and reuse of the exchange
    buffers, a frame-plan step between two batches), also after set_choppiness and set_spectrum;
  * times that are no ramp.

Everything is compared on the device (float32 viewed as int32: a NaN equals itself, -0 differs from +0); only the oracle cases copy a
frame to the host.  Times are fixed per step index, t_k = 0.125 + 0.61 k, so one set of 32 single-step references serves every batch
size of a grid."""
import collections

import numpy as np
import pytest

import p1_groups
import workloads

pytestmark = pytest.mark.gpu

SEED = 6                                   # the handles of test_every_kind_of_batch_size_equals_single_steps
MAXB = p1_groups.MAX_BATCH
TIMES = [0.125 + 0.61 * k for k in range(MAXB)]
FILL = -1                                  # int32 all ones: a NaN in every float

Frames = collections.namedtuple("Frames", "v n w")      # [slots][N*N][3], [slots][N*N][3], [slots][N*N] or [slots][N*N][4]


def make(mw, p, seed=SEED):
    return mw.Ocean(resolution=p.N, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y),
                    amplitude=p.amplitude, choppiness=p.choppiness, gravity=p.gravity, seed=seed)


def bits(a):
    import torch
    return a.view(torch.int32)


class Slots:
    """Output buffers of `nslots` steps with a guard slot in front of slot 0 and one behind the last: the enqueue gets the pointer of
    slot 0 inside the larger allocation (slot sizes are multiples of 16 bytes at every FFT grid size)."""

    def __init__(self, nslots, NN, rgba=False):
        import torch
        self.nslots, self.rgba = nslots, rgba
        self.all = Frames(torch.empty((nslots + 2, NN, 3), dtype=torch.float32, device="cuda"),
                          torch.empty((nslots + 2, NN, 3), dtype=torch.float32, device="cuda"),
                          torch.empty((nslots + 2, NN, 4) if rgba else (nslots + 2, NN), dtype=torch.float32, device="cuda"))
        assert all(a[1].data_ptr() % 16 == 0 for a in self.all)

    def fill(self):
        for a in self.all:
            bits(a).fill_(FILL)

    def enqueue(self, o, times):
        """Fill, then enqueue `times` into slot 0 onwards.  The fills run on torch's stream, the handle enqueues on its own non-blocking
        stream: the device is idle in between."""
        import torch
        self.fill()
        torch.cuda.synchronize()
        self.enqueue_only(o, times)

    def enqueue_only(self, o, times):
        assert len(times) <= self.nslots
        o.evaluate_device(times, self.all.v[1].data_ptr(), self.all.n[1].data_ptr(), self.all.w[1].data_ptr(), rgba=self.rgba)

    def check(self, ref, ns, tag, first=0):
        """Slots [0, ns) equal ref[first : first + ns] bit for bit in all three arrays (colour output: all four channels equal the
        reference's scalar whitecap); every other slot and both guards still hold the fill."""
        for name, a, r in zip(("vertices", "normals", "whitecap"), self.all, ref):
            a, r = bits(a), bits(r)[first:first + ns]
            if name == "whitecap" and self.rgba:
                r = r.unsqueeze(-1).expand(-1, -1, 4)
            bad = (a[1:1 + ns] != r).flatten(1).any(1).nonzero().flatten().tolist()
            assert not bad, f"{tag}: {name} of steps {bad} differ from the same times enqueued alone"
            wrote = (a[1 + ns:-1] != FILL).flatten(1).any(1).nonzero().flatten().tolist()
            assert not wrote, f"{tag}: {name} written in slots {[ns + k for k in wrote]}, which the enqueue was not asked for"
            assert bool((a[0] == FILL).all()), f"{tag}: {name} written in front of slot 0"
            assert bool((a[-1] == FILL).all()), f"{tag}: {name} written behind slot {self.nslots - 1}"


def singles(o, times, NN, into=None):
    """Every time of `times` enqueued alone on o (evaluate_device with one step) -> Frames [len(times)], on the device."""
    import torch
    ref = into or Frames(torch.empty((len(times), NN, 3), dtype=torch.float32, device="cuda"),
                         torch.empty((len(times), NN, 3), dtype=torch.float32, device="cuda"),
                         torch.empty((len(times), NN), dtype=torch.float32, device="cuda"))
    for a in ref:
        bits(a).fill_(FILL)
    torch.cuda.synchronize()
    for k, t in enumerate(times):
        o.evaluate_device([t], ref.v[k].data_ptr(), ref.n[k].data_ptr(), ref.w[k].data_ptr())
    o.synchronize()
    return ref


def assert_live(ref, tag):
    """The references are frames of a moving sea: finite, some whitecap, neighbouring times different in every array -- a pass on frames
    that do not depend on t is ruled out."""
    import torch
    assert all(bool(torch.isfinite(a).all()) for a in ref), tag
    assert bool((ref.w != 0).flatten(1).any(1).all()), f"{tag}: a frame without any whitecap"
    for a in ref:
        assert bool((bits(a)[1:] != bits(a)[:-1]).flatten(1).any(1).all()), f"{tag}: two neighbouring times gave the same frame"


def time_group(mw, o, ns):
    return int(mw.lib().mw_debug_pass1_time_group(o.handle, ns))


@pytest.fixture(scope="module")
def references(mw):
    """N -> the 32 single-step frames of the default handle (seed 6, workloads.fftmesh_params(N)) at TIMES, computed once per grid on a
    handle that never runs a batch, checked to be live, never written again; released with the module."""
    import torch
    cache = {}

    def get(N):
        if N not in cache:
            p = workloads.fftmesh_params(N)
            with make(mw, p) as o:
                assert o.max_batch == MAXB
                cache[N] = singles(o, TIMES, N * N)
            assert_live(cache[N], f"references N={N}")
        return cache[N]

    yield get
    cache.clear()
    torch.cuda.empty_cache()


# ---- a. every batch size, every step ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [64, 128, 256, 512, 1024, 2048])
def test_every_batch_size_every_step(mw, references, N):
    """ns = 1 .. 32, one enqueue each of t_0 .. t_{ns-1} into 32-slot buffers: 528 (ns, step) pairs per grid, all three arrays, the
    untouched slots and the guards.  ns = 1, 11, 13, 17, 19, 23, 29, 31 run the plain grid of pass 1, the others groups of 2 .. 8."""
    import torch
    ref = references(N)
    out = Slots(MAXB, N * N)
    plain = []
    with make(mw, workloads.fftmesh_params(N)) as o:
        for ns in range(1, MAXB + 1):
            tg = time_group(mw, o, ns)
            assert tg == p1_groups.time_group(ns), (N, ns)
            plain += [ns] * (tg == 0)
            out.enqueue(o, TIMES[:ns])
            o.synchronize()
            out.check(ref, ns, f"N={N} ns={ns} (time group {tg})")
    assert plain == [1, 11, 13, 17, 19, 23, 29, 31]
    del out
    torch.cuda.empty_cache()


# ---- b. 4096^2, and d. at 4096^2 ---------------------------------------------------------------------------------------------------

def check_one_by_one(o_ref, out, times, tag, one):
    """Slots.check with the references computed one at a time into the one-slot buffers `one` (the large grid): every step of `times`
    against the same time alone on o_ref, then the rest of the buffer."""
    import torch
    ns = len(times)
    for k, t in enumerate(times):
        singles(o_ref, [t], one.v.shape[1], into=one)
        assert all(bool(torch.isfinite(a).all()) for a in one) and bool((one.w != 0).any()), (tag, k)
        for name, a, r in zip(("vertices", "normals", "whitecap"), out.all, one):
            r = bits(r)[0]
            if name == "whitecap" and out.rgba:
                r = r.unsqueeze(-1).expand(-1, 4)
            assert torch.equal(bits(a)[1 + k], r), f"{tag}: {name} of step {k} differ from the same time enqueued alone"
    for name, a in zip(("vertices", "normals", "whitecap"), out.all):
        for k in range(ns - 1):      # ... which are frames of a moving sea: neighbouring steps differ
            assert not torch.equal(bits(a)[1 + k], bits(a)[2 + k]), f"{tag}: {name} of steps {k} and {k + 1} are the same frame"
        for s in range(ns, out.nslots):
            assert bool((bits(a)[1 + s] == FILL).all()), f"{tag}: {name} written in slot {s}, which the enqueue was not asked for"
        assert bool((bits(a)[0] == FILL).all()) and bool((bits(a)[-1] == FILL).all()), f"{tag}: {name} written outside the buffer"


def one_slot(NN):
    import torch
    return Frames(torch.empty((1, NN, 3), dtype=torch.float32, device="cuda"), torch.empty((1, NN, 3), dtype=torch.float32, device="cuda"),
                  torch.empty((1, NN), dtype=torch.float32, device="cuda"))


def test_every_step_at_4096(mw):
    """4096^2 (no frame plan: a single step is the batched kernels with nsteps = 1, oracle-gated by test_fftmesh_large_grids): batches of
    5, 8, 11 and 12 steps -- time groups of 5 and 8, the plain grid, groups of 6 -- every step, 36 (ns, step) pairs, into 12-slot buffers
    with guards (about 12 GB on the device with the exchange buffers of 12 steps); the references one at a time."""
    import torch
    N = 4096
    NN = N * N
    one = one_slot(NN)
    out = Slots(12, NN)
    with make(mw, workloads.fftmesh_params(N)) as o:
        for ns, want in ((5, 5), (8, 8), (11, 0), (12, 6)):
            assert time_group(mw, o, ns) == p1_groups.time_group(ns) == want
            out.enqueue(o, TIMES[:ns])
            o.synchronize()
            check_one_by_one(o, out, TIMES[:ns], f"N=4096 ns={ns} (time group {want})", one)
    del out, one
    torch.cuda.empty_cache()


def test_colour_output_every_step_at_4096(mw):
    """4096^2, 9 steps (time groups of 3) with MW_OUT_COLOR_RGBA into 10 slots of [N^2][4] with guards: all four channels of every step
    equal the scalar whitecap of the same time alone."""
    import torch
    N = 4096
    NN = N * N
    one = one_slot(NN)
    out = Slots(10, NN, rgba=True)
    with make(mw, workloads.fftmesh_params(N)) as o:
        out.enqueue(o, TIMES[:9])
        o.synchronize()
        check_one_by_one(o, out, TIMES[:9], "N=4096 ns=9, colour output", one)
    del out, one
    torch.cuda.empty_cache()


# ---- c. the MW_P1_TGROUP switch -------------------------------------------------------------------------------------------------

GROUP_OF_24 = {0: 0, 2: 2, 3: 3, 4: 4, 5: 4, 6: 6, 7: 6, 8: 8}      # cap -> time group of a 24-step enqueue


class capped:
    """A handle created with MW_P1_TGROUP = cap (the switch is read when a handle is created); the switch is back at -1 on leaving."""

    def __init__(self, mw, p, cap):
        self.mw, self.p, self.cap = mw, p, cap

    def __enter__(self):
        try:
            self.mw.set_switch("MW_P1_TGROUP", self.cap)
            self.o = make(self.mw, self.p)
        finally:
            self.mw.set_switch("MW_P1_TGROUP", -1)
        return self.o

    def __exit__(self, *a):
        self.o.close()


@pytest.mark.parametrize("N", [128, 1024])
def test_time_group_switch_changes_no_bit(mw, references, N):
    """Caps 0 (the plain grid for every batch size) and 2 .. 8: batches of 24, 21 and 9 steps under every cap equal the references of
    a default handle, every step -- 24 runs groups of 0, 2, 3, 4, 4, 6, 6, 8, 21 groups of 0, 0, 3, 3, 3, 3, 7, 7, 9 groups of 0 or 3."""
    import torch
    ref = references(N)      # (before the switch moves: the references are a default handle's)
    out = Slots(MAXB, N * N)
    p = workloads.fftmesh_params(N)
    for cap, g24 in GROUP_OF_24.items():
        with capped(mw, p, cap) as o:
            assert mw.get_switch("MW_P1_TGROUP") == -1
            assert time_group(mw, o, 24) == g24 == p1_groups.time_group(24, cap), cap
            for ns in (24, 21, 9):
                tg = time_group(mw, o, ns)
                assert tg == p1_groups.time_group(ns, cap), (cap, ns)
                out.enqueue(o, TIMES[:ns])
                o.synchronize()
                out.check(ref, ns, f"N={N} cap={cap} ns={ns} (time group {tg})")
    with make(mw, p) as o:      # and a handle created afterwards follows the built-in rule again
        assert [time_group(mw, o, ns) for ns in (24, 21, 9)] == [8, 7, 3]
    del out
    torch.cuda.empty_cache()


def test_time_group_switch_changes_no_bit_4096(mw):
    """The same at 4096^2: the plain grid for 8 steps (cap 0) and groups of 4 for 12 steps (cap 4), every step against a default
    handle's single steps."""
    import torch
    N = 4096
    NN = N * N
    p = workloads.fftmesh_params(N)
    one = one_slot(NN)
    out = Slots(12, NN)
    with make(mw, p) as default:
        for cap, ns, want in ((0, 8, 0), (4, 12, 4)):
            with capped(mw, p, cap) as o:
                assert time_group(mw, o, 24) == GROUP_OF_24[cap] and time_group(mw, o, ns) == p1_groups.time_group(ns, cap) == want
                assert time_group(mw, default, ns) == p1_groups.time_group(ns) != want
                out.enqueue(o, TIMES[:ns])
                o.synchronize()
                check_one_by_one(default, out, TIMES[:ns], f"N=4096 cap={cap} ns={ns} (time group {want})", one)
    del out, one
    torch.cuda.empty_cache()


# ---- d. colour output --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [64, 128, 256, 512, 1024, 2048])
def test_colour_output_every_step(mw, references, N):
    """MW_OUT_COLOR_RGBA, 9 steps into [32][N^2][4]: all four channels of every step equal the scalar whitecap of the same time alone,
    vertices and normals as before, the remaining slots and the guards untouched."""
    import torch
    out = Slots(MAXB, N * N, rgba=True)
    with make(mw, workloads.fftmesh_params(N)) as o:
        out.enqueue(o, TIMES[:9])
        o.synchronize()
        out.check(references(N), 9, f"N={N} ns=9, colour output")
    del out
    torch.cuda.empty_cache()


# ---- e. back-to-back enqueues on one handle ----------------------------------------------------------------------------------------

SEQUENCE = ((3, 7), (32, 0), (5, 11), (1, 30), (24, 8), (1, 2), (11, 21))      # (steps, first time index) of the seven enqueues


@pytest.mark.parametrize("N", [256, 1024, 2048])
def test_enqueues_of_different_sizes_back_to_back(mw, oracle, references, N):
    """3, 32, 5, 1, 24, 1 and 11 steps into seven output sets on a fresh handle with no host synchronisation in between, one wait, then
    every step of every set: the exchange buffers grow (3 -> 32: ensure_exchange waits for the stream and reallocates), are reused by
    smaller batches, and at 256^2 / 1024^2 the one-step enqueues in the middle run the frame plan's kernels on them.  Every enqueue
    starts elsewhere on the time ramp, so a set that kept another enqueue's frames does not pass.  Then the same sequence on the same
    handle after set_choppiness and after set_spectrum with an oracle spectrum; the references of those states are single steps of a
    second handle that runs no batch."""
    import torch
    NN = N * N
    p = workloads.fftmesh_params(N)
    sets = [Slots(ns, NN) for ns, _ in SEQUENCE]
    ref = references(N)
    h0, h0c = oracle.generate_spectrum(p, 23)
    with make(mw, p) as o, make(mw, p) as r:
        for state in ("fresh", "choppiness", "spectrum"):
            if state == "choppiness":
                o.set_choppiness(1.1); r.set_choppiness(1.1)
            elif state == "spectrum":
                o.set_spectrum(h0, h0c); r.set_spectrum(h0, h0c)
            if state != "fresh":
                before, ref = ref, singles(r, TIMES, NN)
                assert_live(ref, f"N={N} {state}")
                # the state moved every frame (the vertices: normals and whitecap do not depend on the choppiness)
                assert bool((bits(ref.v) != bits(before.v)).flatten(1).any(1).all()), state
                del before
            for s in sets:
                s.fill()
            torch.cuda.synchronize()
            for s, (ns, first) in zip(sets, SEQUENCE):
                s.enqueue_only(o, TIMES[first:first + ns])
            o.synchronize()
            for j, (s, (ns, first)) in enumerate(zip(sets, SEQUENCE)):
                s.check(ref, ns, f"N={N} {state}: enqueue {j} of {[n for n, _ in SEQUENCE]}", first=first)
    del sets, ref
    torch.cuda.empty_cache()


# ---- f. times that are not a ramp ----------------------------------------------------------------------------------------------------

ODD_TIMES = [5.5, 0.0, -2.25, 3600.0, 1.75, 0.125, 1.75, 17.0, 0.61, 3.0e-3, 42.0, 0.3]      # unsorted; 1.75 twice; < 0; 0; an hour


@pytest.mark.parametrize("N", [128, 1024])
def test_times_that_are_not_a_ramp(mw, N):
    """One 12-step batch (time groups of 6) of unsorted times with a repeated entry, a negative one, 0.0 and 3600.0: every slot equals its
    own time enqueued alone, the two slots of the repeated time equal each other."""
    import torch
    NN = N * N
    assert ODD_TIMES[4] == ODD_TIMES[6] and sorted(ODD_TIMES) != ODD_TIMES and min(ODD_TIMES) < 0 and 0.0 in ODD_TIMES and 3600.0 in ODD_TIMES
    out = Slots(12, NN)
    with make(mw, workloads.fftmesh_params(N)) as o, make(mw, workloads.fftmesh_params(N)) as r:
        ref = singles(r, ODD_TIMES, NN)
        assert all(bool(torch.isfinite(a).all()) for a in ref) and bool((ref.w != 0).flatten(1).any(1).all())
        distinct = [k for k in range(12) if k != 6]
        for a in ref:      # different times, different frames
            assert all(not torch.equal(bits(a)[i], bits(a)[j]) for i in distinct for j in distinct if i < j)
        out.enqueue(o, ODD_TIMES)
        o.synchronize()
        out.check(ref, 12, f"N={N}, times {ODD_TIMES}")
        for a in out.all:
            assert torch.equal(bits(a)[1 + 4], bits(a)[1 + 6])
    del out, ref
    torch.cuda.empty_cache()


# ---- g. interior steps against the float64 oracle ------------------------------------------------------------------------------------

@pytest.mark.parametrize("N", [128, 2048])
@pytest.mark.parametrize("ns,k", [(8, 3), (11, 5)])
def test_interior_steps_vs_oracle_f64(mw, oracle, N, ns, k):
    """An independent reference for steps that are neither the first nor the last of their pass-1 time group: step 3 of an 8-step batch
    (interior to a group of 8) and step 5 of an 11-step batch (the plain grid) against oracle.eval_fft_f64 at the project's stated
    tolerances (workloads.assert_parity, as test_batched_enqueue_at_the_timed_shapes_vs_oracle calls it)."""
    import torch
    NN = N * N
    p = workloads.fftmesh_params(N)
    rest = oracle.rest_mesh(p)[0]
    out = Slots(ns, NN)
    with make(mw, p) as o:
        assert time_group(mw, o, ns) == {8: 8, 11: 0}[ns]
        h0, h0c = o.get_spectrum()
        out.enqueue(o, TIMES[:ns])
        o.synchronize()
    v, n, w = (a[1 + k].cpu().numpy() for a in out.all)
    del out
    torch.cuda.empty_cache()
    vf, nf, cf, hds = oracle.eval_fft_f64(p, h0, h0c, np.float32(TIMES[k]), return_hds=True)
    workloads.assert_parity(v, n, w[:, None], vf, nf, cf[:, :1], rest, np.abs(hds).max(), tag=f"N={N} step {k} of {ns}", hds=hds)
