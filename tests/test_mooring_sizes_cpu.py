"""CPU tier of the moorings at the hull chunk and LDS edges (csrc/fleet.h: k_fleet_step, the strict one-launch loop a moored call runs with its lines; the
plan rule of moored_one_launch).  The GPU tier (tests/test_mooring_sizes_gpu.py) compares the device bit for bit with a chain that holds no
device value -- mooring_ref.chain: per substep the rows of an ordered g++ shim (tests/periodic_shim.cpp, tests/draught_shim.cpp), then
one substep of tests/moorings_shim.cpp.  Here that chain is itself checked, over the synthetic periodic mesh periodic_synth(64, 1.0, 0.5)
with the edge hulls t257 (2 chunks) and t40_v600 (3 chunks, two of them without a triangle), 4 substeps of h = 0.05, drag on:

* the launch arithmetic: MW_MOORED_LDS_STATIC = 416 B, the one-launch plan ends at 5055 vertices with 20 chunks (step bodies': 5068);
* every substep of the chain against float64, from the chain's own state: the rows against hull_ref.forces on the same vertex slab within
  test_hull_sizes_cpu's 1e-4 S, and the stepped state against mooring_ref.step fed the float64 row within what those row bounds, the
  wrench bounds of test_moorings_cpu (TOL_F S_F, TOL_TAU S_tau) and the integrator's 4e-6 (1 + |x|) (test_bodies_cpu) allow together:
      v: h / m (b_F + TOL_F S_F) + 4e-6 (1 + |v|)        w: h |I_w^-1| sqrt(3) (b_tau + TOL_TAU S_tau) + 4e-6 (1 + |w|)
      p: h e_v + 4e-6 (1 + |p|)                          q: h e_w + 4e-6 (1 + |q|)
  (sqrt(3): a bound on every entry of a 3-vector bounds its 2-norm, which |I_w^-1| acts on).  No bound is new;
* the sum of those per-substep bounds over the call is the scale the final state is held to.  A chain that loses one sentinel triangle,
  or one taut slot, ends at least 100 times that away in some block of every body, so the bit comparisons of the GPU tier cannot
  miss either;
* the conditions the scenes have to meet (mooring_ref.scene_is_live)."""
import numpy as np
import pytest

import body_ref as B
import hull_ref as H
import mooring_ref as M
import periodic_ref as PR
import test_hull_sizes_cpu as THC
import test_moorings_cpu as TC
from test_hull_sizes_cpu import mesh, shim  # noqa: F401  (fixtures)
from test_moorings_cpu import ms  # noqa: F401  (the moorings shim, as a fixture)

RHO, G = THC.RHO, THC.G
R, UW = THC.R, THC.UW
LIN, QUAD = 30.0, 60.0
DT, SUB, K = 0.2, 4, 8
NAMES = ["t257", "t40_v600"]
# the moored one-launch plan's LDS edge: name -> (ntris, nverts, cells of the barge, chunks)
EDGE = {"v5055": (5120, 5055, (46, 46), 20), "v5056": (5120, 5056, (46, 46), 20)}
BLOCKS = (("p", slice(0, 3)), ("q", slice(4, 8)), ("v", slice(8, 11)), ("w", slice(12, 15)))
_hulls = {}


def hull_of(name):
    """test_hull_sizes_cpu's edge hulls, and v5055 / v5056"""
    if name not in EDGE:
        return THC.hull_of(name)
    if name not in _hulls:
        ntris, nverts, cells, _ = EDGE[name]
        _hulls[name] = H.edge_hull(ntris, nverts, cells)
    return _hulls[name]


def edge_mass(mw, n, rng):
    """test_hull_sizes_gpu._mass: a 6 x 1.5 x 6 box of 20 to 30 t"""
    m = rng.uniform(20000.0, 30000.0, n)
    return mw.pack_mass(m, np.array([B.box_inertia(k, 6.0, 1.5, 6.0) for k in m]))


# ---- launch arithmetic ----------------------------------------------------------------------------------------------------------
def test_the_moored_one_launch_plan_ends_at_5055_vertices(shim, ms):  # noqa: F811
    top = shim.ps_bodies_lds_max()
    assert ms.ms_moored_lds_static() == 416
    assert shim.ps_bodies_step_lds(5055, 20) + 416 == top
    assert shim.ps_bodies_step_lds(5056, 20) + 416 == top + 32
    assert shim.ps_bodies_step_lds(5068, 20) == top                               # step bodies' own edge lies 13 vertices above
    for name, (ntris, nverts, _, chunks) in EDGE.items():
        x, t = hull_of(name)
        assert (len(x), len(t)) == (nverts, ntris) and t.min() >= 0 and t.max() < len(x)
        assert shim.ps_hull_chunks(len(x), len(t)) == chunks == 20


# ---- the chain against float64 --------------------------------------------------------------------------------------------------
class Scene:
    """3 moored bodies of an edge hull afloat on the tiling of the synthetic mesh, the last in the neighbouring tile"""

    def __init__(self, mw, shim, mesh, name):  # noqa: F811
        self.shim, self.mesh = shim, mesh
        self.hull, self.tris = hull_of(name)
        self.P = PR.period(R, UW)
        self.bodies = THC.poses(shim, mesh, self.P, 3, seed=len(name) + 30)
        rng = np.random.default_rng(len(name) + 34)
        self.mass = edge_mass(mw, 3, rng)
        self.h = float(np.float32(DT) / np.float32(SUB))
        self.lines, self.kind = M.moor(mw, rng, self.bodies, self.mass, K, self.h, self.P)
        self.cf = np.array([RHO, G, LIN, QUAD, 1.0], np.float32)

    def run(self, ms, tris=None, lines=None):  # noqa: F811
        """(chain result, the trace, the vertex slab of every substep)"""
        tris = self.tris if tris is None else tris
        slabs, trace = [], []

        def rows_of(b):
            slab, rows = PR.hull_forces(self.shim, R, UW, self.P, self.mesh["vert"], self.mesh["vel"], self.hull, tris, b, self.cf)
            slabs.append(slab)
            return rows
        want = M.chain(ms, rows_of, self.bodies, self.mass, self.lines if lines is None else lines, G, DT, SUB, trace)
        return want, trace, slabs


_scenes = {}


def _audit(s, want, trace, slabs):
    """every substep from the chain's own state against float64: records (substep, body, what, error, bound) of the rows and of the four
    blocks of the stepped state, and per block the sum of the bounds over the call [3 bodies]"""
    records, total = [], {key: np.zeros(len(s.bodies)) for key, _ in BLOCKS}
    for k, (b0, rows, T) in enumerate(trace):
        b1 = trace[k + 1][0] if k + 1 < SUB else want[0]
        for j in range(len(b0)):
            ref, per = THC.reference(slabs[k][j], s.tris, b0[j], LIN, QUAD)
            bf, ba, bt = THC.bounds(per)
            err = np.abs(rows[j, :7] - ref)
            records += [(k, j, "F", err[0:3].max(), bf), (k, j, "A", err[3], ba), (k, j, "tau", err[4:7].max(), bt)]
            row = np.zeros(8)
            row[:7] = ref
            mrow = s.mass[j].astype(np.float64)
            nxt = M.step(b0[j], row, mrow, s.lines[j], G, s.h)
            _, _, _, SF, ST = M.wrenches(b0[j:j + 1], s.lines[j:j + 1])
            Rm = H.rotation(b0[j:j + 1, 4:8])[0]
            Iw_inv = np.linalg.norm(Rm @ np.linalg.inv(B.inertia_matrix(mrow)) @ Rm.T, 2)
            ev = s.h / mrow[0] * (bf + TC.TOL_F * SF[0]) + 4e-6 * (1 + np.abs(nxt[8:11]).max())
            ew = s.h * Iw_inv * np.sqrt(3.0) * (bt + TC.TOL_TAU * ST[0]) + 4e-6 * (1 + np.abs(nxt[12:15]).max())
            bound = dict(p=s.h * ev + 4e-6 * (1 + np.abs(nxt[0:3]).max()), q=s.h * ew + 4e-6 * (1 + np.abs(nxt[4:8]).max()), v=ev, w=ew)
            for key, sl in BLOCKS:
                records.append((k, j, key, np.abs(b1[j, sl] - nxt[sl]).max(), bound[key]))
                total[key][j] += bound[key]
    return records, total


@pytest.fixture
def scene(mw, shim, mesh, ms, request):  # noqa: F811
    """(the scene, its chain, the audit of that chain), computed once per hull"""
    name = request.param
    if name not in _scenes:
        s = Scene(mw, shim, mesh, name)
        run = s.run(ms)
        _scenes[name] = (s, run, _audit(s, *run))
    return _scenes[name]


@pytest.mark.parametrize("scene", NAMES, indirect=True)
def test_every_substep_of_the_chain_against_float64(scene):
    s, (want, trace, slabs), (records, total) = scene
    assert len(trace) == len(slabs) == SUB and len(records) == SUB * 3 * 7
    for k, j, what, err, bound in records:
        print("substep %d body %d %s: err/bound %.2e" % (k, j, what, err / bound))
    for k, j, what, err, bound in records:
        assert err <= bound, (k, j, what, err, bound)
    for (b0, _, _), b1 in zip(trace, [t[0] for t in trace[1:]] + [want[0]]):
        assert np.array_equal(b1[:, [3, 11, 15]], b0[:, [3, 11, 15]])
    assert abs(s.bodies[2, 0]) > 40.0                                             # one body in the neighbouring tile


# ---- a lost piece moves the answer ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", NAMES, indirect=True)
def test_a_lost_sentinel_or_slot_moves_the_final_state_by_100_bounds(scene, ms):  # noqa: F811
    s, (want, trace, _), (_, total) = scene
    T0 = trace[0][2]
    assert (T0.max(1) > 0).all()
    emptied = s.lines.copy()
    for j in range(len(s.bodies)):                                                # every body loses the slot that pulls hardest at the start
        emptied[j, int(np.argmax(T0[j])), 7:9] = 0.0
    cases = [("slot", dict(lines=emptied))]
    for k in H.sentinel_slots(len(s.tris)):
        less = s.tris.copy()
        less[k] = 0                                                               # a degenerate triangle: no area, no force
        cases.append(("sentinel %d" % k, dict(tris=less)))
    for what, kw in cases:
        got = s.run(ms, **kw)[0][0]
        for j in range(len(s.bodies)):
            moved = {key: np.abs(got[j, sl].astype(np.float64) - want[0][j, sl]).max() / total[key][j] for key, sl in BLOCKS}
            print(what, j, " ".join("%s %.0f" % kv for kv in moved.items()))
            assert max(moved.values()) >= 100.0, (what, j, moved)


# ---- a NaN row ------------------------------------------------------------------------------------------------------------------
def test_a_nan_row_leaves_the_body_and_reports_nan_tensions(mw, ms):  # noqa: F811
    """the header's rule for a failed body, whatever made it fail: its state stays and its tensions are NaN beside its NaN row -- also
    for a NaN position, whose lines mooring_slot would otherwise all report slack (l > L0 is false for a NaN l)"""
    bodies = mw.pack_bodies([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [np.nan, 0.0, 0.0]])
    mass = edge_mass(mw, 3, np.random.default_rng(0))
    lines = mw.pack_lines(3, 2, anchor=[[[0.0, -5.0, 0.0], [3.0, -4.0, 0.0]]] * 3, rest_length=[[1.0, 50.0]], stiffness=1e4, damping=10.0)
    rows = np.zeros((3, 8), np.float32)
    rows[1, 5] = np.nan
    rows[2] = np.nan
    b = bodies.copy()
    T, ok = TC.step(ms, b, rows, mass, lines, G, 0.01)
    assert list(ok) == [1, 0, 0] and T[0, 0] > 0 and T[0, 1] == 0
    assert np.isnan(T[1:]).all() and np.array_equal(TC._bits(b[1:]), TC._bits(bodies[1:])) and not np.array_equal(b[0], bodies[0])


# ---- scene conditions ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", NAMES, indirect=True)
def test_the_scenes_are_live(scene, ms):  # noqa: F811
    s, (want, trace, _), _ = scene
    M.scene_is_live(ms, s.bodies, s.lines, want, trace, len(H.sentinel_slots(len(s.tris))), wet_throughout=True)
    assert (s.kind[:, 0] == M.TAUT).all() and {M.EMPTY, M.SLACK, M.TAUT} <= set(s.kind.ravel())
    kinds = M.slots(s.bodies, s.lines)[0]
    assert np.array_equal(kinds, s.kind)                                          # float64 agrees on which slot is which
    assert s.h * np.sqrt(8 * s.lines[:, :, 7].max(1) / s.mass[:, 0]).max() < 0.2
    assert (np.abs(s.lines[:, :, 0:3]) <= [3.0, 0.75, 3.0]).all()                 # attachment points inside the box
