"""GPU tier of the moorings (mw_ocean_step_moored / _device, include/mistral_water.h) through the C ABI, on small oceans: FFTMesh 64^2 and
OceanRenderer resolution 8; the hulls are hull_ref.box (12 triangles) and icosphere(subdiv=1) (80 triangles).

* a periodic handle: states, out and tension after 8 substeps equal, bit for bit, the chain of tests/moorings_shim.cpp's substep fed the
  device's own rows (mw_ocean_hull_forces_device at every intermediate state) -- both plans, host and device forms, drag off and on,
  1, 255, 256 and 257 bodies (the last lane of k_moored_integrate's first workgroup and the first of its second), K = 1 and 8;
* the two plans give the same bits; every line slack or empty gives mw_ocean_step_bodies' bits (periodic, and non-periodic with
  draught); one substep equals mw_ocean_step_fleet_device given the shim's wrench; the first substep's out is
  mw_ocean_hull_forces_device's; 257 bodies, slack, taut and one invalid, through both plans, the one-launch plan being the
  fleets' k_fleet_step on a one-hull table;
* a moored box on flat water surges with the period of its lines; invalid slots and NaN rows stay local; the argument, frame and state
  rules; the handle's state is untouched;
* the one footprint without draught, whose rows come from kernels built with contraction, against the float64 composition.
Hulls of more than one chunk, the one-launch plan's LDS edge, K = 2 .. 7 and taut lines under draught: tests/test_mooring_sizes_gpu.py.

Measured on an MI355X (this file's seeds): the footprint check's worst error is 2.41e-5 of the displacement over the call for p (an ulp of
|p| ~ 20 against 0.04 moved), 3.18e-6 of the change over the call for v, 3.33e-6 for w and 2.62e-6 for q; the asserted bounds are 8x those
figures rounded up."""
import ctypes as C

import numpy as np
import pytest

import body_ref as B
import hull_ref as H
import mooring_ref as M
import surface_ref as S
import test_moorings_cpu as TC
import workloads
from test_moorings_cpu import ms  # noqa: F401  (the shim, as a fixture)

pytestmark = pytest.mark.gpu
RHO, G = 1000.0, 9.81
DRAG = dict(linear_drag=30.0, quadratic_drag=60.0)
P = 64.0  # the period of the 64^2 sea
# 8x the measured error of the footprint check, relative to each block's change over the call (test_footprint_against_float64 prints it)
FOOT = dict(p=8 * 2.5e-5, v=8 * 3.2e-6, w=8 * 3.4e-6, q=8 * 2.7e-6)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ocean(mw, periodic=False, t=1.7, frame=True, flat=False, choppiness=1.0):
    p = workloads.fftmesh_params(64, choppiness=choppiness)
    o = mw.Ocean(resolution=p.N, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                 choppiness=p.choppiness, gravity=p.gravity, seed=3, device=0)
    if flat:  # a zero spectrum: every vertex at its rest position, height 0 (test_bodies_gpu._flat)
        z = np.zeros((o.N, o.N, 2), np.float32)
        o.set_spectrum(z, z)
    if frame:
        o.evaluate(t)
    if periodic:
        o.set_periodic(True)
    return o


def _renderer(mw):
    o = mw.Ocean(resolution=8, unit_width=1.0, length=27.155, wind=(14.45, 12.0), amplitude=0.41, choppiness=1.5, mult=1.5, seed=1,
                 semantics=mw.MW_SEM_OCEANRENDERER, device=0)
    for dt in (0.3, 0.4):
        o.generate_texture(dt)
    return o


def _hull(mw, name):
    """(hull about its centre of mass, triangles, one mass row) of a named hull at 600 kg/m^3"""
    x, t = H.box(1.5, 1.0, 2.0) if name == "box" else H.icosphere(1.2, 1)
    m, c, I = mw.hull_mass_properties(x, t, 600.0)
    return np.asarray(x - c, np.float32), t, mw.pack_mass(m, I)


def _scene(mw, o, rng, n, K, span, hull_name="box", slack=False, poses=None):
    """n moving bodies near the water within +-span (3 x 3 tiles of a periodic sea for span = 96; o None: near y = 0; poses: (p, q) given)
    and their lines, every anchor 3 to 6 below and beside its body, in the body's own tile: K = 1 one taut line; K = 8
    the first slot taut and the others a mix of taut, slack and empty.  slack: every slot slack or empty."""
    hull, tris, mrow = _hull(mw, hull_name)
    if poses is None:
        pos = np.stack([rng.uniform(-span, span, n), np.zeros(n), rng.uniform(-span, span, n)], 1).astype(np.float32)
        if o is not None:
            pos[:, 1] = o.query_surface(np.ascontiguousarray(pos[:, [0, 2]]), mode="world")[:, 1]
        pos[:, 1] += rng.uniform(-0.3, 0.3, n)
        quat = H.upright_quaternions(n, rng, 25.0)
    else:
        pos, quat = poses
    bodies = mw.pack_bodies(pos, quat, rng.standard_normal((n, 3)) * 0.5, rng.standard_normal((n, 3)) * 0.3)
    mass = np.repeat(mrow, n, 0)
    u = rng.standard_normal((n, K, 3))
    u[:, :, 1] = -np.abs(u[:, :, 1])  # the anchors lie below
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    dist = rng.uniform(3.0, 6.0, (n, K))
    kind = rng.choice([M.EMPTY, M.SLACK, M.TAUT], (n, K))
    kind[:, 0] = M.TAUT
    if slack:
        kind = np.where(kind == M.TAUT, M.SLACK, kind)
    m = float(mrow[0, 0])
    off = u * dist[:, :, None]
    # an anchor stays in its body's tile of the 64-periodic sea (tiles are [-32 + 64 k, 32 + 64 k)): an offset that leaves it is mirrored
    xz = np.asarray(pos, np.float64)[:, None, [0, 2]]
    leaves = np.floor((xz + 32.0) / P) != np.floor((xz + off[:, :, [0, 2]] + 32.0) / P)
    off[:, :, 0] = np.where(leaves[:, :, 0], -off[:, :, 0], off[:, :, 0])
    off[:, :, 2] = np.where(leaves[:, :, 1], -off[:, :, 2], off[:, :, 2])
    # |h| <= 0.52 < 0.2 * 3: a taut slot (L0 = 0.8 dist) is taut and a slack one (1.5 dist) slack wherever the body points
    lines = mw.pack_lines(n, K, attach=rng.uniform(-0.3, 0.3, (n, K, 3)), anchor=np.asarray(pos)[:, None, :] + off,
                          rest_length=dist * np.where(kind == M.SLACK, 1.5, 0.8),
                          stiffness=np.where(kind == M.EMPTY, 0.0, rng.uniform(2.0, 6.0, (n, K)) * m),   # h sqrt(8 k / m) < 0.2
                          damping=np.where(kind == M.EMPTY, 0.0, rng.uniform(0.0, 1.0, (n, K)) * m))
    return hull, tris, bodies, mass, lines


def _up(*arrays):
    import torch
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]
    torch.cuda.synchronize()
    return d


def _moored_device(o, hull, tris, bodies, mass, lines, dt, substeps, **kw):
    import torch
    d_h, d_t, d_b, d_m, d_l = _up(hull, tris, bodies.copy(), mass, lines)
    d_o = torch.full((len(bodies), 8), 7.0, dtype=torch.float32, device="cuda")
    d_n = torch.full(lines.shape[:2], 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    o.step_moored_device(d_h.data_ptr(), len(hull), d_t.data_ptr(), len(tris), d_b.data_ptr(), d_m.data_ptr(), d_l.data_ptr(), lines.shape[1],
                         len(bodies), dt, substeps, d_out=d_o.data_ptr(), d_tension=d_n.data_ptr(), **kw)
    o.synchronize()
    return d_b.cpu().numpy(), d_o.cpu().numpy(), d_n.cpu().numpy()


def _moored_host(o, hull, tris, bodies, mass, lines, dt, substeps, **kw):
    return o.step_moored(hull, tris, bodies.copy(), mass, lines, dt, substeps=substeps, return_forces=True, return_tension=True, **kw)


def _forces_device(o, hull, tris, bodies, **kw):
    import torch
    d_h, d_t, d_b = _up(hull, tris, bodies)
    d_o = torch.zeros((len(bodies), 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    o.hull_forces_device(d_h.data_ptr(), len(hull), d_t.data_ptr(), len(tris), d_b.data_ptr(), len(bodies), d_o.data_ptr(), **kw)
    o.synchronize()
    return d_o.cpu().numpy()


def _chain(ms, o, hull, tris, bodies, mass, lines, dt, substeps, **kw):  # noqa: F811
    """the shim's substep chain fed the device's own rows: (state, the last row, the last tensions)"""
    h = float(np.float32(dt) / np.float32(substeps))
    b = bodies.copy()
    for _ in range(substeps):
        rows = _forces_device(o, hull, tris, b, **kw)
        T, ok = TC.step(ms, b, rows, mass, lines, G, h)
    return b, rows, T


def _run_plan(mw, value, fn):
    old = mw.get_switch("MW_BODIES_PLAN")
    mw.set_switch("MW_BODIES_PLAN", value)
    try:
        return fn()
    finally:
        mw.set_switch("MW_BODIES_PLAN", old)


@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_device_equals_the_shim_bit_for_bit(mw, ms, n, K):  # noqa: F811
    rng = np.random.default_rng(10 * n + K)
    with _ocean(mw, periodic=True) as o:
        hull, tris, bodies, mass, lines = _scene(mw, o, rng, n, K, 96.0)
        for kw in ({}, DRAG):
            want = _chain(ms, o, hull, tris, bodies, mass, lines, 0.16, 8, **kw)
            assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and (want[2][:, 0] > 0).any()
            assert not _same(want[0][:, 0:3], bodies[:, 0:3])
            for plan in (0, 1):
                for form in (_moored_host, _moored_device):
                    got = _run_plan(mw, plan, lambda: form(o, hull, tris, bodies, mass, lines, 0.16, 8, **kw))
                    for g, w, what in zip(got, want, ("state", "out", "tension")):
                        bad = np.nonzero((_bits(g) != _bits(w)).reshape(n, -1).any(1))[0]
                        assert len(bad) == 0, (what, plan, form.__name__, bool(kw), bad[:5], g[bad[:2]], w[bad[:2]])


@pytest.mark.parametrize("hull_name", ["box", "icosphere"])
def test_plans_give_the_same_bits(mw, hull_name):
    rng = np.random.default_rng(21)
    with _ocean(mw, periodic=True) as o:
        hull, tris, bodies, mass, lines = _scene(mw, o, rng, 64, 8, 96.0, hull_name)
        for kw in ({}, DRAG):
            a = _run_plan(mw, 0, lambda: _moored_host(o, hull, tris, bodies, mass, lines, 0.16, 8, **kw))
            b = _run_plan(mw, 1, lambda: _moored_host(o, hull, tris, bodies, mass, lines, 0.16, 8, **kw))
            assert all(_same(x, y) for x, y in zip(a, b)) and np.isfinite(a[0]).all() and (a[2] > 0).any()
            free = o.step_bodies(hull, tris, bodies.copy(), mass, 0.16, substeps=8, **kw)
            assert not _same(a[0], free)  # the lines pull


def test_all_slack_equals_step_bodies(mw):
    """every line slack or empty: mw_ocean_step_bodies' bits on a periodic handle (both plans) and on a non-periodic handle with draught
    (4 layers), where both calls integrate strictly.  On the plain footprint mw_ocean_step_bodies' k_bodies_integrate<SqMesh> is built
    with contraction and the moored integration is strict, so the two are held together by the footprint check's tolerance instead."""
    rng = np.random.default_rng(22)
    with _ocean(mw, periodic=True) as o:
        hull, tris, bodies, mass, lines = _scene(mw, o, rng, 40, 8, 96.0, slack=True)
        for kw in ({}, DRAG):
            for plan in (0, 1):
                got, rows, T = _run_plan(mw, plan, lambda: _moored_host(o, hull, tris, bodies, mass, lines, 0.16, 8, **kw))
                free, frows = _run_plan(mw, plan, lambda: o.step_bodies(hull, tris, bodies.copy(), mass, 0.16, substeps=8, return_forces=True, **kw))
                assert _same(got, free) and _same(rows, frows) and (T == 0).all() and not _same(got, bodies)
    with _ocean(mw) as o:
        hull, tris, bodies, mass, lines = _scene(mw, o, rng, 40, 8, 24.0, slack=True)
        plain = {}
        for draught in (True, False):
            if draught:
                o.set_column([0.0, 0.5, 1.5, 4.0])
                o.set_draught(True)
            else:
                o.set_draught(False)
            for name, kw in (("off", {}), ("on", DRAG)):
                got, rows, T = _moored_host(o, hull, tris, bodies, mass, lines, 0.16, 8, **kw)
                free, frows = o.step_bodies(hull, tris, bodies.copy(), mass, 0.16, substeps=8, return_forces=True, **kw)
                assert (T == 0).all() and np.isfinite(got).all()
                if draught:
                    assert _same(got, free) and _same(rows, frows)
                else:
                    plain[name] = (got, free)
        start = bodies
        for name, (got, free) in plain.items():
            for key, sl in (("p", slice(0, 3)), ("v", slice(8, 11)), ("w", slice(12, 15)), ("q", slice(4, 8))):
                change = np.linalg.norm(free[:, sl].astype(np.float64) - start[:, sl], axis=1)
                err = np.abs(got[:, sl].astype(np.float64) - free[:, sl]).max(1)
                assert (err <= FOOT[key] * change).all(), (name, key, (err / change).max())


def test_moored_calls_ride_the_fleet_table(mw):
    """The one-launch plan of a moored call is the fleets' strict k_fleet_step on a one-hull table, with the lines; the per-substep plan
    is k_moored_integrate.  257 boxes, K = 8, 3 substeps: the last body sits in the second 256-lane workgroup of the per-substep kernel.
    Every third body's lines are all slack or empty, body 130 has an invalid slot, the rest are taut.  The two plans give equal states,
    out and tension to the bit, the NaN pattern included, and the slack bodies are mw_ocean_step_bodies_device's to the bit."""
    import torch
    n, K, bad = 257, 8, 130
    with _ocean(mw, periodic=True) as o:
        # the same draws twice: the two scenes differ in the rest lengths alone
        hull, tris, bodies, mass, taut = _scene(mw, o, np.random.default_rng(24), n, K, 96.0)
        slack = _scene(mw, o, np.random.default_rng(24), n, K, 96.0, slack=True)
        assert _same(bodies, slack[2])
        loose = np.arange(n) % 3 == 0
        lines = np.where(loose[:, None, None], slack[4], taut).astype(np.float32)
        assert not loose[bad] and not loose[n - 1]
        lines[bad, 3, 7] = -1.0  # a negative stiffness
        hauled = ~loose & (np.arange(n) != bad)
        got = {}
        for plan in (1, 0):
            got[plan] = _run_plan(mw, plan, lambda: _moored_device(o, hull, tris, bodies, mass, lines, 0.06, 3))
            d_h, d_t, d_b, d_m = _up(hull, tris, bodies.copy(), mass)
            d_o = torch.full((n, 8), 7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            _run_plan(mw, plan, lambda: o.step_bodies_device(d_h.data_ptr(), len(hull), d_t.data_ptr(), len(tris), d_b.data_ptr(), d_m.data_ptr(), n,
                                                             0.06, 3, d_o.data_ptr()))
            o.synchronize()
            state, out, tens = got[plan]
            free, frows = d_b.cpu().numpy(), d_o.cpu().numpy()
            assert _same(state[loose], free[loose]) and _same(out[loose], frows[loose]) and (tens[loose] == 0).all(), plan
            assert not _same(free[loose], bodies[loose])
            assert _same(state[bad], bodies[bad]) and np.isnan(out[bad]).all() and np.isnan(tens[bad]).all(), plan
            assert np.isfinite(state[hauled]).all() and np.isfinite(out[hauled]).all() and (tens[hauled] >= 0).all(), plan
            # the lines pull: slot 0 is taut by its length, and only a fast approach can clamp its tension to 0
            assert (tens[hauled, 0] > 0).mean() > 0.9 and ((_bits(state[hauled]) != _bits(free[hauled])).any(1)).mean() > 0.9, plan
        for a, b, what in zip(got[1], got[0], ("state", "out", "tension")):
            assert _same(a, b), what  # equal bits: a NaN in one plan is the same NaN in the other


@pytest.mark.parametrize("plan", [0, 1], ids=["per_substep", "one_launch"])
def test_one_substep_equals_step_fleet_with_the_shims_wrench(mw, ms, plan):  # noqa: F811
    import torch
    rng = np.random.default_rng(23)
    with _ocean(mw, periodic=True) as o:
        hull, tris, bodies, mass, lines = _scene(mw, o, rng, 70, 8, 96.0)
        wr, T, taut = TC.wrench(ms, bodies, lines)
        assert (taut == 1).all()  # every body has a taut line: the fleet call always adds its wrench
        x, t, table = mw.pack_fleet([(hull, tris, len(bodies))])
        for lin, quad in ((0.0, 0.0), (30.0, 60.0)):
            cf = o._hull_coeffs(RHO, G, lin, quad, None)[None]
            d_x, d_t, d_b, d_m, d_w = _up(x, t, bodies.copy(), mass, wr)
            d_o = torch.zeros((len(bodies), 8), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()

            def fleet():
                o.step_fleet_device(d_x.data_ptr(), len(x), d_t.data_ptr(), len(t), table, d_b.data_ptr(), d_m.data_ptr(), len(bodies), 0.02, 1,
                                    d_wrench=d_w.data_ptr(), d_out=d_o.data_ptr(), coeffs=cf)
                o.synchronize()
                return d_b.cpu().numpy(), d_o.cpu().numpy()
            fb, fo = _run_plan(mw, plan, fleet)
            got, rows, tens = _run_plan(mw, plan, lambda: _moored_device(o, hull, tris, bodies, mass, lines, 0.02, 1, linear_drag=lin,
                                                                          quadratic_drag=quad))
            assert _same(got, fb) and _same(rows, fo) and _same(tens, T) and not _same(got, bodies)


@pytest.mark.parametrize("surface", ["periodic", "footprint", "renderer"])
def test_first_substep_out_is_hull_forces(mw, surface):
    rng = np.random.default_rng(24)
    o, span = (_renderer(mw), 2.0) if surface == "renderer" else (_ocean(mw, periodic=surface == "periodic"), 24.0)
    with o:
        hull, tris, bodies, mass, lines = _scene(mw, o, rng, 30, 8, span)
        if surface == "renderer":
            hull = (hull * 0.3).astype(np.float32)
        for kw in ({}, DRAG):
            want = _forces_device(o, hull, tris, bodies, **kw)
            got, rows, T = _moored_device(o, hull, tris, bodies, mass, lines, 0.02, 1, **kw)
            assert _same(rows, want) and np.isfinite(want).all() and (want[:, 3] > 0).any() and not _same(got, bodies)


def test_moored_box_surges_on_flat_water(mw):
    """a floating box (half the water's density: centre at the waterline) between two opposing taut horizontal lines at the height of its
    centre of mass, drag off: the surge period is 2 pi sqrt(m / 2k) to 1 % while the heave stays at equilibrium; both plans"""
    x, t = H.box(2.0, 1.0, 3.0)
    m = 500.0 * 6.0
    mass = mw.pack_mass(m, B.box_inertia(m, 2.0, 1.0, 3.0))
    k, D, L0, x0 = 3000.0, 20.0, 10.0, 0.5
    Tp = 2 * np.pi * np.sqrt(m / (2 * k))
    lines = mw.pack_lines(1, 2, anchor=[[[D, 0.0, 0.0], [-D, 0.0, 0.0]]], rest_length=L0, stiffness=k)
    dt, K = 0.032, 4
    assert dt / K * np.sqrt(2 * k / m) <= 0.1
    with _ocean(mw, periodic=True, flat=True) as o:
        for plan in (0, 1):
            b = mw.pack_bodies([[x0, 0.0, 0.0]])
            xs, ys, ts = [x0], [0.0], [0.0]

            def run():
                while ts[-1] < 3.3 * Tp:
                    o.step_moored(x, t, b, mass, lines, dt, substeps=K)
                    xs.append(float(b[0, 0])); ys.append(float(b[0, 1])); ts.append(ts[-1] + dt)
            _run_plan(mw, plan, run)
            xa, ta = np.array(xs), np.array(ts)
            kk = np.nonzero((xa[:-1] > 0) & (xa[1:] <= 0))[0]  # downward crossings
            tc = ta[kk] + (ta[kk + 1] - ta[kk]) * xa[kk] / (xa[kk] - xa[kk + 1])
            assert len(tc) >= 3
            period = (tc[-1] - tc[0]) / (len(tc) - 1)
            assert abs(period - Tp) <= 0.01 * Tp, (plan, period, Tp)
            assert 0.9 * x0 <= xa.max() <= 1.01 * x0 and -1.01 * x0 <= xa.min() <= -0.9 * x0
            assert np.abs(ys).max() < 1e-3 and abs(b[0, 2]) < 1e-3


def test_invalid_slots_and_nan_rows_stay_local(mw):
    rng = np.random.default_rng(25)
    with _ocean(mw, periodic=True) as o:
        hull, tris, bodies, mass, lines = _scene(mw, o, rng, 5, 8, 96.0)
        j = 2
        others = [0, 1, 3, 4]
        for slot, k, value in ((3, 0, np.nan), (7, 7, -1.0), (0, 5, np.inf)):
            bad = lines.copy()
            bad[j, slot, k] = value
            bad[j, slot, 9:12] = np.nan  # the padding is not read, here or in the other bodies
            bad[0, 0, 9:12] = np.nan
            with pytest.raises(mw.MistralWaterError) as e:
                o.step_moored(hull, tris, bodies.copy(), mass, bad, 0.16, substeps=8)
            assert e.value.status == mw.MW_EINVAL and ("slot %d of body %d" % (slot, j)).encode() in mw.lib().mw_last_error()
            for plan in (0, 1):
                want = _run_plan(mw, plan, lambda: _moored_device(o, hull, tris, bodies[others], mass[others], lines[others], 0.16, 8))
                got = _run_plan(mw, plan, lambda: _moored_device(o, hull, tris, bodies, mass, bad, 0.16, 8))
                assert np.isnan(got[1][j]).all() and np.isnan(got[2][j]).all() and _same(got[0][j], bodies[j])
                assert all(_same(g[others], w) for g, w in zip(got, want)) and np.isfinite(want[0]).all()
        # a NaN row: a non-finite pose keeps its bits and reports a NaN row; a pose turning non-finite mid-call freezes where it was
        nb = bodies.copy()
        nb[1, 0] = np.nan
        nb[3, 12:15] = [1e30, 2e30, -1e30]
        for plan in (0, 1):
            got, rows, T = _run_plan(mw, plan, lambda: _moored_host(o, hull, tris, nb, mass, lines, 0.16, 8))
            assert _same(got[1], nb[1]) and np.isnan(rows[1]).all() and np.isnan(rows[3]).all()
            assert np.isfinite(rows[[0, 2, 4]]).all() and np.isfinite(got[[0, 2, 4]]).all()
            b = nb[3:4].copy()
            for _ in range(8):  # one substep per call until the row is NaN: the state there is the frozen one
                prev = b.copy()
                b, rb, _ = _moored_host(o, hull, tris, b, mass[3:4], lines[3:4], float(np.float32(0.16) / np.float32(8)), 1)
                if np.isnan(rb).any():
                    assert _same(b, prev)
                    break
            else:
                pytest.fail("the pose never turned non-finite")
            assert _same(got[3], b[0])


def test_argument_checks(mw):
    import torch
    L = mw.lib()
    hull, tris, mrow = _hull(mw, "box")
    body = mw.pack_bodies([[0.0, 0.0, 0.0]])
    lines = mw.pack_lines(1, 2, anchor=[[[0.0, -5.0, 0.0]] * 2], rest_length=1.0, stiffness=100.0)
    cf = np.array([RHO, G, 0, 0, 1], np.float32)
    out, ten = np.zeros((1, 8), np.float32), np.zeros((1, 2), np.float32)
    with _ocean(mw) as o:
        h = o._h

        def call(sub=1, dt=0.1, mm=_p(mrow), ll=_p(lines), K=2, oo=_p(out), tt=_p(ten), nb=1, frame=-1):
            return L.mw_ocean_step_moored(h, frame, _p(hull), 8, _p(tris), 12, _p(body), mm, ll, K, nb, _p(cf), C.c_float(dt), sub, 0, oo, tt)
        assert call() == mw.MW_OK and call(oo=None, tt=None) == mw.MW_OK and call(nb=0, ll=None) == mw.MW_OK
        before = body.copy()
        for kw in (dict(sub=0), dict(sub=65), dict(dt=-0.1), dict(dt=float("nan")), dict(dt=float("inf")), dict(mm=None), dict(frame=0),
                   dict(nb=-1), dict(K=0), dict(K=9), dict(K=-1), dict(ll=None)):
            assert call(**kw) == mw.MW_EINVAL, kw
        assert _same(body, before)
        assert call(sub=64) == mw.MW_OK and call(dt=0.0) == mw.MW_OK
        buf = torch.zeros(64 * 40, dtype=torch.float32, device="cuda")
        base = buf.data_ptr()
        for off_b, off_m, off_l, off_o, off_t, want in ((0, 0, 0, 0, 0, mw.MW_OK), (4, 0, 0, 0, 0, mw.MW_EINVAL), (0, 8, 0, 0, 0, mw.MW_EINVAL),
                                                         (0, 0, 8, 0, 0, mw.MW_EINVAL), (0, 0, 0, 4, 0, mw.MW_EINVAL), (0, 0, 0, 0, 2, mw.MW_EINVAL),
                                                         (0, 0, 0, 0, 4, mw.MW_OK)):
            s = L.mw_ocean_step_moored_device(h, -1, C.c_void_p(base + 4096), 8, C.c_void_p(base + 5120), 12, C.c_void_p(base + off_b),
                                              C.c_void_p(base + 1024 + off_m), C.c_void_p(base + 6144 + off_l), 2, 1, _p(cf), C.c_float(0.1),
                                              1, 0, C.c_void_p(base + 2048 + off_o), C.c_void_p(base + 3072 + off_t))
            assert s == want, (off_b, off_m, off_l, off_o, off_t)
        o.synchronize()


def test_frame_and_state_rules(mw, oracle):
    hull, tris, mass = _hull(mw, "box")
    body = mw.pack_bodies([[0.3, 0.0, -0.2]])
    lines = mw.pack_lines(1, 1, anchor=[[[0.3, -6.0, -0.2]]], rest_length=4.0, stiffness=500.0, damping=50.0)
    p = workloads.fftmesh_params(64, choppiness=1.0)

    def status(o, **kw):
        b = body.copy()
        with pytest.raises(mw.MistralWaterError) as e:
            o.step_moored(hull, tris, b, mass, lines, 0.1, **kw)
        assert _same(b, body)  # caller arrays untouched on failure
        return e.value.status
    with _ocean(mw, frame=False) as o:
        assert status(o) == mw.MW_ESTATE  # no frame yet
        o.evaluate(1.0)
        o.step_moored(hull, tris, body.copy(), mass, lines, 0.1, linear_drag=1.0)
        h0, h0c = oracle.generate_spectrum(p, 3)
        o.set_spectrum(h0, h0c)
        o.step_moored(hull, tris, body.copy(), mass, lines, 0.1)  # drag off: the surface query's rules
        assert status(o, quadratic_drag=1.0) == mw.MW_ESTATE       # drag on: the velocity query's
        o.evaluate(1.2)
        o.set_draught(True)
        assert status(o) == mw.MW_ESTATE                           # draught on and no column
        o.set_column([0.0, 1.0, 3.0])
        o.step_moored(hull, tris, body.copy(), mass, lines, 0.1)
        o.set_periodic(True)                                        # the periodic and the draught switch combine as in step_bodies
        a = o.step_moored(hull, tris, body.copy(), mass, lines, 0.1, substeps=4)
        b = o.step_bodies(hull, tris, body.copy(), mass, 0.1, substeps=4)
        assert np.isfinite(a).all() and not _same(a, b)
    with _renderer(mw) as r:
        r.generate_texture_steps([0.05, 0.1, 0.07])
        small = (hull * 0.3).astype(np.float32)
        outs = [r.step_moored(small, tris, body.copy(), mass, lines, 0.05, frame=k) for k in range(3)]
        assert not _same(outs[0], outs[2])
        r.step_moored(small, tris, body.copy(), mass, lines, 0.05, frame=2, linear_drag=3.0)
        with pytest.raises(mw.MistralWaterError) as e:
            r.step_moored(small, tris, body.copy(), mass, lines, 0.05, frame=1, linear_drag=3.0)
        assert e.value.status == mw.MW_EINVAL


def test_step_moored_changes_no_state(mw):
    """timer, frames, queries and the periodic, draught and column switches are what they are without the moored calls"""
    rng = np.random.default_rng(1)
    xz = np.ascontiguousarray(rng.uniform(-30, 30, (50, 2)), np.float32)
    xyz = np.ascontiguousarray(np.concatenate([xz, rng.uniform(-3, 0, (50, 1)).astype(np.float32)], 1)[:, [0, 2, 1]])

    def run(with_moored):
        out = []
        with _ocean(mw, frame=False) as o:
            o.set_column([0.0, 1.0, 2.5])
            for k in range(3):
                v, n, c = o.update(0.03)
                o.set_periodic(k == 1)
                o.set_draught(k == 2)
                if with_moored:
                    hull, tris, bodies, mass, lines = _scene(mw, None, np.random.default_rng(2), 8, 8, 20.0)
                    o.step_moored(hull, tris, bodies.copy(), mass, lines, 0.1, substeps=4)
                    o.step_moored(hull, tris, bodies.copy(), mass, lines, 0.1, substeps=4, **DRAG)
                out += [v, n, c, np.float32(o.timer), np.float32(o.periodic), np.float32(o.draught), o.column,
                        o.query_surface(xz, mode="world"), o.query_velocity(xz, mode="world"), o.query_column(xyz)]
        return out

    a, b = run(False), run(True)
    assert len(a) == len(b) and all(_same(np.atleast_1d(x), np.atleast_1d(y)) for x, y in zip(a, b))

    def run_renderer(with_moored):  # OceanRenderer: the phase, and the frame made from it
        with _renderer(mw) as r:
            if with_moored:
                hull, tris, bodies, mass, lines = _scene(mw, None, np.random.default_rng(3), 6, 8, 2.0)
                small = (hull * 0.3).astype(np.float32)
                r.step_moored(small, tris, bodies.copy(), mass, lines, 0.1, substeps=4)
                r.step_moored(small, tris, bodies.copy(), mass, lines, 0.1, substeps=4, **DRAG)
            return [r.get_phase(), *r.generate_texture(0.1), r.get_phase()]

    a, b = run_renderer(False), run_renderer(True)
    assert all(_same(x, y) for x, y in zip(a, b))


def _eta64(vert, tris, xz):
    """float64 water height at xz [n, 2] on the displaced mesh vert [R*R, 3] (the triangle that holds the point; None where none does)"""
    hits = S.world_hits(xz, vert, tris, 1e-12)
    out = np.full(len(xz), np.nan)
    for k, (t, w) in enumerate(hits):
        if len(t):
            out[k] = (w[0] * vert[tris[t[0]], 1]).sum()
    return out


def test_footprint_against_float64(mw, oracle):
    """A non-periodic handle without draught: hull_launch's rows come from the kernels built with contraction, so the states after 8
    substeps are held to the float64 composition -- hull_ref.forces on the oracle's float64 frame of the same spectrum, mooring_ref, and
    body_ref.step -- relative to each block's change over the call.  A body whose world-mode residual exceeds 1e-4 unit widths is left
    out, at most 1 % of them; the reference finds a triangle for every vertex at every substep."""
    p = workloads.fftmesh_params(64, choppiness=0.46)
    h0, h0c = oracle.generate_spectrum(p, 3)
    vert = oracle.eval_fft_f64(p, h0, h0c, 1.7)[0].astype(np.float64)
    tris_w = S.grid_triangles(p.N)
    rng = np.random.default_rng(26)
    n, K, dt, sub = 24, 8, 0.16, 8
    with _ocean(mw, frame=False, choppiness=0.46) as o:
        o.set_spectrum(h0, h0c)
        o.evaluate(1.7)
        eta = lambda xz: _eta64(vert, tris_w, np.asarray(xz, np.float64))  # noqa: E731
        hull, tris, bodies, mass, lines = _scene(mw, o, rng, n, K, 20.0, poses=H.afloat_poses(n, rng, 20.0, eta))
        got, rows, T = _moored_host(o, hull, tris, bodies, mass, lines, dt, sub)
    h = float(np.float32(dt) / np.float32(sub))
    ref = bodies.astype(np.float64)
    for _ in range(sub):
        x = H.transform(ref, hull)
        e = _eta64(vert, tris_w, x.reshape(-1, 3)[:, [0, 2]]).reshape(n, -1)
        assert np.isfinite(e).all()  # the reference alone leaves out none
        for b in range(n):
            row = np.zeros(8)
            row[:7] = H.forces(x[b], e[b] - x[b, :, 1], np.zeros_like(x[b]), tris, ref[b], RHO, G)
            ref[b] = M.step(ref[b], row, mass[b].astype(np.float64), lines[b], G, h)
    keep = rows[:, 7] <= 1e-4 * p.unit_width
    assert (~keep).sum() <= 0.01 * n and np.isfinite(got).all() and (T > 0).any()
    for key, sl in (("p", slice(0, 3)), ("v", slice(8, 11)), ("w", slice(12, 15)), ("q", slice(4, 8))):
        change = np.linalg.norm(ref[:, sl] - bodies[:, sl], axis=1)
        err = np.abs(got[:, sl] - ref[:, sl]).max(1)
        print("footprint %s: worst error %.3e of the change over the call (smallest change %.3e)" % (key, (err / change)[keep].max(), change.min()))
    for key, sl in (("p", slice(0, 3)), ("v", slice(8, 11)), ("w", slice(12, 15)), ("q", slice(4, 8))):
        change = np.linalg.norm(ref[:, sl] - bodies[:, sl], axis=1)
        err = np.abs(got[:, sl] - ref[:, sl]).max(1)
        assert (err[keep] <= FOOT[key] * change[keep]).all(), (key, (err / change)[keep].max())
