"""GPU tier of the moorings (mw_ocean_step_moored / _device) at the hull chunk and LDS edges and with taut lines under draught, through the
C ABI, on FFTMesh 64^2, unit_width 1, one frame.

The reference is mooring_ref.chain: per substep the rows of an ordered g++ shim at the current state (tests/periodic_shim.cpp on a
periodic handle, tests/draught_shim.cpp with draught on), then one substep of tests/moorings_shim.cpp.  It holds no device value but the
frame arrays read back from the handle, so it sees an error the rows and the moored kernels would share; tests/test_mooring_sizes_cpu.py
holds it to float64 and shows that a lost sentinel or slot moves it by a hundred bounds.  Every comparison here is bit for bit.

1. a periodic handle, the edge hulls of tests/test_hull_sizes_gpu.py (255 / 256 / 257 triangles, 40 triangles on 600 vertices, 16 385
   triangles: 1, 1, 2, 3 and 65 chunks), the plans MW_BODIES_PLAN = 1, 0 and -1, host and device forms, drag off and on;
2. the moored one-launch plan's LDS edge: v5055 (bodies_step_lds + 416 B = MW_BODIES_LDS_MAX, the largest slab k_fleet_step is
   launched with for a moored call), v5056 (32 B above: a forced plan 1 steps per substep) and v5068 (step bodies' own edge);
3. K = 1 .. 8: which lanes stage the slots and store the tensions, with a canary behind [nbodies][K];
4. substeps = 1 and 64;
5. taut lines under draught: periodic and non-periodic handle, 2 and 5 layers, the spar, the icosphere and t257, with the NaN pose, the
   hull in the air and the hull below the deepest layer of test_draught_gpu._poses;
6. the one footprint without draught: the rows come from kernels built with contraction, the integration is the strict
   k_moored_integrate, so the call equals the chain of the moorings shim fed mw_ocean_hull_forces_device's rows;
7. failures stay local on a multi-chunk hull: a NaN vertex, an invalid slot."""
import numpy as np
import pytest

import draught_ref as DR
import hull_ref as H
import mooring_ref as M
import periodic_ref as PR
import test_draught_gpu as TD
import test_hull_sizes_gpu as THS
import test_mooring_sizes_cpu as TMC
import test_moorings_gpu as TG
import test_periodic_gpu as TP
import workloads
from test_hull_sizes_gpu import shim  # noqa: F401  (the periodic shim, as a fixture)
from test_moorings_cpu import ms  # noqa: F401  (the moorings shim, as a fixture)

pytestmark = pytest.mark.gpu
bits = PR.bits
G = 9.81
DT, SUB = 0.2, 4        # h = 0.05, test_hull_sizes_gpu's stepping
H_LINES = 0.05          # the substep the lines' stiffness is scaled for (mooring_ref.moor): h <= H_LINES in every case


def hull_of(name):
    return TMC.hull_of(name) if name in TMC.EDGE else THS.hull_of(name)


@pytest.fixture(scope="module")
def dshim(tmp_path_factory):
    return DR.build_shim(str(tmp_path_factory.mktemp("msg") / "libdraught_shim.so"))


def _equal(got, want, tag):
    """state, out and tension of a call against the chain's, bit for bit (a NaN for a NaN, whatever its payload)"""
    for g, w, what in zip(got, want, ("state", "out", "tension")):
        assert g.shape == w.shape, (tag, what, g.shape, w.shape)
        same = (bits(g) == bits(w)) | (np.isnan(g) & np.isnan(w))
        bad = np.nonzero(~same.reshape(len(w), -1).all(1))[0]
        assert len(bad) == 0, (tag, what, bad[:5], g[bad[:2]], w[bad[:2]])


def _nsent(tris):
    return len(H.sentinel_slots(len(tris)))


class Sea:
    """a periodic 64^2 handle, its frame arrays, and n moored bodies of an edge hull afloat on it, the last in a neighbouring tile"""

    def __init__(self, mw, name, n, K, seed, h=H_LINES):
        self.mw = mw
        self.hull, self.tris = hull_of(name)
        self.o, self.m = THS._sea(mw, True)
        self.bodies = THS._afloat(mw, self.o, n, seed=seed, shift=(-self.m["P"], self.m["P"]))
        rng = np.random.default_rng(seed + 1000)
        self.mass = THS._mass(mw, n, rng)
        self.lines, self.kind = M.moor(mw, rng, self.bodies, self.mass, K, h, self.m["P"])

    def chain(self, pshim, ms, drag, dt=DT, substeps=SUB, hull=None, bodies=None, mass=None, lines=None):  # noqa: F811
        m = self.m
        kw, cf = THS._coeffs(self.o, drag)
        hull = self.hull if hull is None else hull
        rows_of = lambda b: PR.hull_forces(pshim, m["R"], m["uw"], m["P"], m["vert"], m["vel"], hull, self.tris, b, cf)[1]  # noqa: E731
        self.trace = []
        return kw, M.chain(ms, rows_of, self.bodies if bodies is None else bodies, self.mass if mass is None else mass,
                           self.lines if lines is None else lines, G, dt, substeps, self.trace)

    def call(self, form, plan, kw, dt=DT, substeps=SUB, hull=None, bodies=None, mass=None, lines=None):
        args = (self.o, self.hull if hull is None else hull, self.tris, self.bodies if bodies is None else bodies,
                self.mass if mass is None else mass, self.lines if lines is None else lines, dt, substeps)
        return TP._run_plan(self.mw, plan, lambda: form(*args, **kw))


# ---- 1. periodic handle, multi-chunk hulls, every plan ---------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("t255", 4), ("t256", 4), ("t257", 4), ("t40_v600", 4), ("t16385", 2)])
def test_periodic_edge_hulls_equal_the_chain_in_every_plan(mw, shim, ms, name, n):  # noqa: F811
    """t16385 asks plan 1 for 9230 + 65 rows of LDS, more than fits: it steps per substep whatever the switch says"""
    s = Sea(mw, name, n, 8, seed=len(name) + 50)
    with s.o:
        assert abs(s.bodies[-1, 0]) > 40.0                                        # one body in the neighbouring tile
        for drag in (False, True):
            kw, want = s.chain(shim, ms, drag)
            M.scene_is_live(ms, s.bodies, s.lines, want, s.trace, _nsent(s.tris))
            for plan in (1, 0, -1):
                for form in (TG._moored_host, TG._moored_device):
                    _equal(s.call(form, plan, kw), want, (name, drag, plan, form.__name__))


# ---- 2. the moored LDS edge ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["v5055", "v5056", "v5068"])
def test_the_moored_lds_edge(mw, shim, ms, name):  # noqa: F811
    """v5055: 162 400 B of dynamic LDS beside k_fleet_step's static arrays, the documented limit -- a refused launch would be an error
    status, which the wrappers raise.  v5056 and v5068 (where step bodies still takes one launch) must step per substep under a forced
    plan 1.  Which plan ran is not visible through the ABI: the bits and the statuses are what is asserted."""
    s = Sea(mw, name, 2, 8, seed=len(name) + 60)
    with s.o:
        kw, want = s.chain(shim, ms, True)
        M.scene_is_live(ms, s.bodies, s.lines, want, s.trace, _nsent(s.tris))
        for plan in ((1,) if name == "v5068" else (1, 0, -1)):
            for form in (TG._moored_host, TG._moored_device):
                _equal(s.call(form, plan, kw), want, (name, plan, form.__name__))


# ---- 3. every K ------------------------------------------------------------------------------------------------------------------
def _device_with_canary(o, hull, tris, bodies, mass, lines, dt, substeps, **kw):
    """TG._moored_device with K + 8 floats more behind the tensions, all of it filled with a canary: (state, out, tension, the rest)"""
    import torch
    n, K = lines.shape[:2]
    d_h, d_t, d_b, d_m, d_l = TG._up(hull, tris, bodies.copy(), mass, lines)
    d_o = torch.full((n, 8), 7.0, dtype=torch.float32, device="cuda")
    d_n = torch.full((n * K + K + 8,), -77.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    o.step_moored_device(d_h.data_ptr(), len(hull), d_t.data_ptr(), len(tris), d_b.data_ptr(), d_m.data_ptr(), d_l.data_ptr(), K, n, dt,
                         substeps, d_out=d_o.data_ptr(), d_tension=d_n.data_ptr(), **kw)
    o.synchronize()
    t = d_n.cpu().numpy()
    return d_b.cpu().numpy(), d_o.cpu().numpy(), t[:n * K].reshape(n, K), t[n * K:]


@pytest.mark.parametrize("K", range(1, 9))
def test_every_k(mw, shim, ms, K):  # noqa: F811
    s = Sea(mw, "t257", 3, K, seed=70 + K)
    with s.o:
        assert s.lines.shape == (3, K, 12)
        kw, want = s.chain(shim, ms, True)
        M.scene_is_live(ms, s.bodies, s.lines, want, s.trace, _nsent(s.tris))
        for plan in (1, 0):
            *got, rest = s.call(_device_with_canary, plan, kw)
            _equal(got, want, (K, plan))
            assert len(rest) == K + 8 and (rest == np.float32(-77.0)).all(), (K, plan, rest)


# ---- 4. substep edges ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("substeps,dt", [(1, 0.05), (64, 0.64)])
def test_substep_edges(mw, shim, ms, substeps, dt):  # noqa: F811
    """h = 0.05 and 0.01, within the range the lines are scaled for"""
    assert np.float32(dt) / np.float32(substeps) <= np.float32(H_LINES)
    s = Sea(mw, "t257", 3, 8, seed=80 + substeps)
    with s.o:
        for drag in (False, True):
            kw, want = s.chain(shim, ms, drag, dt, substeps)
            M.scene_is_live(ms, s.bodies, s.lines, want, s.trace, _nsent(s.tris))
            for plan in (1, 0):
                for form in (TG._moored_host, TG._moored_device):
                    got = s.call(form, plan, kw, dt, substeps)
                    _equal(got, want, (substeps, drag, plan, form.__name__))
                    if substeps == 1:
                        assert np.array_equal(bits(got[1]), bits(TG._forces_device(s.o, s.hull, s.tris, s.bodies, **kw)))


# ---- 5. taut lines under draught -------------------------------------------------------------------------------------------------
def _draught_hull(mw, name, n, rng):
    """(hull, triangles, how far a vertex lies from p at most plus the way a body makes in the call, the attachment box, mass rows)"""
    if name == "t257":
        hull, tris = hull_of(name)
        return hull, tris, 5.5, (2.7, 0.6, 2.7), THS._mass(mw, n, rng)
    (hull, tris), reach = TD._hull(name)
    return hull, tris, reach + 1.0, (0.9, 7.0, 0.9) if name == "spar" else (0.8, 0.8, 0.8), TD._mass_rows(mw, hull, tris, n)


@pytest.mark.parametrize("periodic", [False, True], ids=["footprint", "periodic"])
@pytest.mark.parametrize("L", [2, 5])
def test_taut_lines_under_draught(mw, dshim, ms, L, periodic):  # noqa: F811
    """7 bodies per hull: four afloat, then test_draught_gpu._poses' NaN pose (it keeps its bits; its row and its tensions are NaN), a
    hull in the air and one below the deepest layer.  8 substeps of h = 0.02.  There is no one-launch plan on the column:
    MW_BODIES_PLAN = 1 changes nothing."""
    p = workloads.fftmesh_params(64, choppiness=1.0)
    depths = TD._depths(L)
    rng = np.random.default_rng(500 + 10 * L + periodic)
    n, dt, sub = 7, 0.16, 8
    with TD._ocean(mw, p) as o:
        o.set_column(depths)
        o.evaluate(1.7)
        if periodic:
            o.set_periodic(True)
        o.set_draught(True)
        pos, vel = TD._layers(o, L)
        P = o.period if periodic else 0.0
        for name in ("spar", "icosphere", "t257"):
            hull, tris, reach, box, mass = _draught_hull(mw, name, n, rng)
            bodies = TD._poses(o, n, rng, periodic, 32.0, depths[-1], reach)
            assert np.isnan(bodies[-3, 0]) and np.isfinite(np.delete(bodies, n - 3, 0)).all()
            finite = bodies.copy()
            finite[-3, 0] = 0.0                                                   # the lines of the NaN pose are valid: its pose is what fails
            lines, kind = M.moor(mw, rng, finite, mass, 8, 0.02, P or None, box)
            assert np.isfinite(lines).all()
            for drag in (False, True):
                cf = TD._coeffs(drag)
                rows_of = lambda b: DR.forces(dshim, 64, 1.0, P, depths, pos, vel, hull, tris, b, cf)[1]  # noqa: E731
                want = M.chain(ms, rows_of, bodies, mass, lines, G, dt, sub)
                state, rows, T = want
                ok = np.arange(n) != n - 3
                assert np.isfinite(state[ok]).all() and np.isfinite(rows[ok]).all() and np.isfinite(T[ok]).all()
                assert (rows[:4, 3] > 0).all() and (T[:4] > 0).any(1).sum() >= 2 and (T[n - 2:] > 0).any()
                assert (bits(state[ok, 0:3]) != bits(bodies[ok, 0:3])).any(1).all()
                assert np.array_equal(bits(state[-3]), bits(bodies[-3])) and np.isnan(rows[-3]).all() and np.isnan(T[-3]).all()
                assert (rows[-2, :7] == 0).all()                                  # in the air: only gravity and the lines
                for plan, form in ((-1, TG._moored_host), (-1, TG._moored_device), (1, TG._moored_device)):
                    got = TP._run_plan(mw, plan, lambda: form(o, hull, tris, bodies, mass, lines, dt, sub, **TD._kw(drag)))
                    _equal(got, want, (name, L, periodic, drag, plan, form.__name__))
                    assert np.array_equal(bits(got[0][-3]), bits(bodies[-3])) and np.isnan(got[1][-3]).all() and np.isnan(got[2][-3]).all()


# ---- 6. the one footprint without draught ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("t257", 4), ("t16385", 2)])
def test_footprint_equals_the_shims_step_on_the_devices_rows(mw, ms, name, n):  # noqa: F811
    """Non-periodic, no draught: hull_launch's rows come from the kernels built with contraction, so no g++ shim has their bits; the
    integration is the strict k_moored_integrate.  The call therefore equals the chain of the moorings shim fed
    mw_ocean_hull_forces_device's rows at every state, and the host form equals the device form."""
    hull, tris = hull_of(name)
    o, m = THS._sea(mw, False)
    with o:
        bodies = THS._afloat(mw, o, n, seed=len(name) + 90)
        rng = np.random.default_rng(len(name) + 91)
        mass = THS._mass(mw, n, rng)
        lines, kind = M.moor(mw, rng, bodies, mass, 8, H_LINES)
        for drag in (False, True):
            kw, _ = THS._coeffs(o, drag)
            trace = []
            want = M.chain(ms, lambda b: TG._forces_device(o, hull, tris, b, **kw), bodies, mass, lines, G, DT, SUB, trace)
            M.scene_is_live(ms, bodies, lines, want, trace, _nsent(tris))
            host = TG._moored_host(o, hull, tris, bodies, mass, lines, DT, SUB, **kw)
            dev = TG._moored_device(o, hull, tris, bodies, mass, lines, DT, SUB, **kw)
            _equal(dev, want, (name, drag, "device"))
            _equal(host, dev, (name, drag, "host against device"))


# ---- 7. failures stay local on a multi-chunk hull --------------------------------------------------------------------------------
def test_a_nan_vertex_freezes_every_body_in_both_plans(mw, shim, ms):  # noqa: F811
    """t40_v600 with its last vertex, which no triangle references, NaN: hull_row's rule makes every row NaN, so k_fleet_step stops
    after its first pass over the three chunks.  Rows and tensions are NaN and no state moves."""
    s = Sea(mw, "t40_v600", 4, 8, seed=100)
    bad = s.hull.copy()
    bad[-1, 2] = np.nan
    assert not (s.tris == len(bad) - 1).any()
    with s.o:
        for drag in (False, True):
            kw, want = s.chain(shim, ms, drag, hull=bad)
            assert np.isnan(want[1]).all() and np.isnan(want[2]).all() and np.array_equal(bits(want[0]), bits(s.bodies))
            for plan in (1, 0):
                for form in (TG._moored_host, TG._moored_device):
                    state, rows, T = s.call(form, plan, kw, hull=bad)
                    assert np.isnan(rows).all() and np.isnan(T).all(), (drag, plan, form.__name__, rows, T)
                    assert np.array_equal(bits(state), bits(s.bodies)), (drag, plan, form.__name__)
            good = s.call(TG._moored_device, 1, kw)                               # the hull itself is sound
            assert np.isfinite(good[1]).all() and not np.array_equal(bits(good[0]), bits(s.bodies))


def test_an_invalid_slot_stays_local_on_a_multi_chunk_hull(mw, shim, ms):  # noqa: F811
    s = Sea(mw, "t40_v600", 4, 8, seed=101)
    j, others = 1, [0, 2, 3]
    bad = s.lines.copy()
    bad[j, 5, 7] = -1.0                                                           # a negative stiffness
    with s.o:
        kw, want = s.chain(shim, ms, True, bodies=s.bodies[others], mass=s.mass[others], lines=s.lines[others])
        assert np.isfinite(want[0]).all() and (want[2] > 0).any()
        for plan in (1, 0):
            three = s.call(TG._moored_device, plan, kw, bodies=s.bodies[others], mass=s.mass[others], lines=s.lines[others])
            _equal(three, want, (plan, "three bodies"))
            got = s.call(TG._moored_device, plan, kw, lines=bad)
            _equal([g[others] for g in got], three, (plan, "the other three"))
            assert np.isnan(got[1][j]).all() and np.isnan(got[2][j]).all() and np.array_equal(bits(got[0][j]), bits(s.bodies[j]))
