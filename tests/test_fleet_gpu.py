"""GPU tier of the mixed fleets (mw_ocean_fleet_forces / mw_ocean_step_fleet and their device forms, include/mistral_water.h) through the
C ABI.  The fleet calls are defined by the single-hull calls: every check here is a comparison of bits with mw_ocean_hull_forces or
mw_ocean_step_bodies on each hull alone (so no tolerance is needed), on small oceans -- FFTMesh 64^2 and OceanRenderer resolution 16.

The standing fleet: a tetrahedron (1 body), a box (65 bodies: more than one reduce workgroup's four waves), an icosphere of 320
triangles (2 chunks), a barge cut to exactly 256 triangles (1 chunk) and the same with one triangle more (2 chunks), 300 vertices with
10 triangles (the chunk count decided by the vertices, 290 of them unreferenced), a barge of 880 triangles (4 chunks: the per-substep
plan under the built-in rule) and one more hull without bodies."""
import ctypes as C
from dataclasses import dataclass

import numpy as np
import pytest

import body_ref as B
import hull_ref as H
import workloads

pytestmark = pytest.mark.gpu
RHO, G = 1000.0, 9.81
NAMES = ("density", "gravity", "linear_drag", "quadratic_drag", "velocity_scale")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _ocean(mw, periodic=False, t=1.7, frame=True):
    p = workloads.fftmesh_params(64, choppiness=1.0)
    o = mw.Ocean(resolution=p.N, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                 choppiness=p.choppiness, gravity=p.gravity, seed=3, device=0)
    if frame:
        o.evaluate(t)
    if periodic:
        o.set_periodic(True)
    return o


def _renderer(mw):
    o = mw.Ocean(resolution=16, unit_width=1.0, length=27.155 * 2, wind=(14.45, 12.0), amplitude=0.41, choppiness=1.5, mult=1.5, seed=1,
                 semantics=mw.MW_SEM_OCEANRENDERER, device=0)
    for dt in (0.3, 0.4):
        o.generate_texture(dt)
    return o


def _surface(mw, kind):
    """(handle, half-width of the square the bodies are spread over) of a named surface"""
    if kind == "renderer":
        return _renderer(mw), 3.0
    if kind == "periodic":
        return _ocean(mw, periodic=True), 96.0  # 3 x 3 tiles of period 64
    return _ocean(mw), 24.0


@dataclass
class Fleet:
    hulls: list        # (hull_xyz, triangles, nbodies)
    bodies: np.ndarray
    mass: np.ndarray
    coeffs: np.ndarray  # [nhulls, 5]

    @property
    def first(self):
        return np.concatenate([[0], np.cumsum([nb for _, _, nb in self.hulls])]).astype(int)

    def rows(self, h):
        return slice(self.first[h], self.first[h + 1])

    def pick(self, order):
        """the fleet of hulls `order` (indices into this one), their bodies with them"""
        idx = np.concatenate([np.arange(self.first[h], self.first[h + 1]) for h in order] + [np.zeros(0, int)]).astype(int)
        return Fleet([self.hulls[h] for h in order], self.bodies[idx].copy(), self.mass[idx].copy(), self.coeffs[list(order)].copy()), idx


def _shapes():
    # a regular tetrahedron, (b - a) x (c - a) pointing out of it
    tet = (np.array([[1, 1, 1], [1, -1, -1], [-1, 1, -1], [-1, -1, 1]], np.float32) * 0.8,
           np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2]], np.int32))
    assert H.volume(*tet) > 0
    gx, gt = H.grid_hull(6, 8, 2.0, 3.0, 0.8)
    assert len(gt) >= 257 and len(gx) < 256
    rng = np.random.default_rng(77)
    loose = rng.uniform(-1.0, 1.0, (300, 3)).astype(np.float32)
    loose_t = np.array([[k, (k + 1) % 10, (k + 2) % 10] for k in range(10)], np.int32)
    bx, bt = H.grid_hull(12, 14, 2.5, 4.0, 1.0)
    assert len(bt) > 768 and (max(len(bt), len(bx)) + 255) // 256 >= 4
    return [tet + (1,), H.box(1.5, 1.0, 2.0) + (65,), H.icosphere(1.2, 2) + (5,), (gx, gt[:256].copy(), 3), (gx, gt[:257].copy(), 3),
            (loose, loose_t, 2), (bx, bt, 2), H.box(1.0, 1.0, 1.0) + (0,)]


def _fleet(mw, span, seed=5, drag="off"):
    """the standing fleet with random poses around the waterline within +-span, a few bodies fully dry and a few fully submerged"""
    rng = np.random.default_rng(seed)
    hulls = _shapes()
    n = sum(nb for _, _, nb in hulls)
    pos = np.stack([rng.uniform(-span, span, n), rng.uniform(-0.6, 0.6, n), rng.uniform(-span, span, n)], 1)
    pos[3::11, 1] = 25.0   # dry
    pos[7::11, 1] = -25.0  # submerged
    bodies = mw.pack_bodies(pos, H.random_quaternions(n, rng), rng.standard_normal((n, 3)), rng.standard_normal((n, 3)) * 0.5)
    bodies[:, [3, 11, 15]] = rng.standard_normal((n, 3)).astype(np.float32)  # the spare floats pass through
    m = rng.uniform(1500.0, 3000.0, n)
    mass = mw.pack_mass(m, np.array([np.diag(rng.uniform(0.6, 1.4, 3)) for _ in range(n)]) * m[:, None, None])
    cf = np.zeros((len(hulls), 5), np.float32)
    cf[:, 0] = rng.uniform(800.0, 1100.0, len(hulls))
    cf[:, 1] = rng.uniform(9.0, 10.0, len(hulls))
    cf[:, 4] = rng.uniform(0.5, 1.5, len(hulls))
    if drag == "each":
        cf[:, 2] = rng.uniform(10.0, 40.0, len(hulls))
        cf[:, 3] = rng.uniform(10.0, 80.0, len(hulls))
        cf[1, 3] = 0.0  # linear only
        cf[2, 2] = 0.0  # quadratic only
    elif drag == "one":
        cf[2, 2:4] = [25.0, 50.0]
    return Fleet(hulls, bodies, mass, cf)


def _kw(cf):
    return {k: float(v) for k, v in zip(NAMES, cf)}


def _single_forces(o, F):
    """mw_ocean_hull_forces on each hull alone, with that hull's coefficients"""
    out = np.zeros((len(F.bodies), 8), np.float32)
    for h, (x, t, nb) in enumerate(F.hulls):
        if nb:
            out[F.rows(h)] = o.hull_forces(x, t, F.bodies[F.rows(h)], **_kw(F.coeffs[h]))
    return out


def _single_step(o, F, dt, substeps):
    b, out = F.bodies.copy(), np.zeros((len(F.bodies), 8), np.float32)
    for h, (x, t, nb) in enumerate(F.hulls):
        if nb:
            s = F.rows(h)
            b[s], out[s] = o.step_bodies(x, t, F.bodies[s].copy(), F.mass[s], dt, substeps=substeps, return_forces=True, **_kw(F.coeffs[h]))
    return b, out


class Dev:
    """a fleet's arrays on the device"""

    def __init__(self, mw, F, wrench=None, tris=None):
        import torch
        self.x, t, self.table = mw.pack_fleet(F.hulls)
        self.t = t if tris is None else tris
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
        self.d_x, self.d_t, self.d_b, self.d_m = up(self.x), up(self.t), up(F.bodies.copy()), up(F.mass)
        self.d_w = None if wrench is None else up(wrench)
        self.d_o = torch.full((len(F.bodies), 8), 7.0, dtype=torch.float32, device="cuda")
        self.cf, self.n = F.coeffs, len(F.bodies)
        torch.cuda.synchronize()

    def forces(self, o):
        o.fleet_forces_device(self.d_x.data_ptr(), len(self.x), self.d_t.data_ptr(), len(self.t), self.table, self.d_b.data_ptr(), self.n,
                              self.d_o.data_ptr(), coeffs=self.cf)

    def step(self, o, dt, substeps):
        o.step_fleet_device(self.d_x.data_ptr(), len(self.x), self.d_t.data_ptr(), len(self.t), self.table, self.d_b.data_ptr(),
                            self.d_m.data_ptr(), self.n, dt, substeps, d_wrench=0 if self.d_w is None else self.d_w.data_ptr(),
                            d_out=self.d_o.data_ptr(), coeffs=self.cf)

    def result(self, o):
        o.synchronize()
        return self.d_b.cpu().numpy(), self.d_o.cpu().numpy()


def _fleet_forces(o, mw, F):
    x, t, table = mw.pack_fleet(F.hulls)
    return o.fleet_forces(x, t, table, F.bodies, coeffs=F.coeffs)


def _step_fleet(o, mw, F, dt, substeps, wrench=None):
    x, t, table = mw.pack_fleet(F.hulls)
    return o.step_fleet(x, t, table, F.bodies.copy(), F.mass, dt, substeps=substeps, wrench=wrench, coeffs=F.coeffs, return_forces=True)


@pytest.fixture(params=[-1, 0, 1], ids=["rule", "per_substep", "one_launch"])
def plan(request, mw):
    old = mw.get_switch("MW_BODIES_PLAN")
    mw.set_switch("MW_BODIES_PLAN", request.param)
    yield request.param
    mw.set_switch("MW_BODIES_PLAN", old)


# ---- 1. rows equal the single-hull calls ------------------------------------------------------------------------------------
@pytest.mark.parametrize("drag", ["off", "each", "one"])
@pytest.mark.parametrize("kind", ["fftmesh", "periodic", "renderer"])
def test_rows_equal_the_single_hull_calls(mw, kind, drag):
    o, span = _surface(mw, kind)
    F = _fleet(mw, span, drag=drag)
    with o:
        want = _single_forces(o, F)
        assert np.isfinite(want).all() and (want[:, 3] > 0).sum() > 40 and (want[:, 3] == 0).any()
        host = _fleet_forces(o, mw, F)
        bad = np.nonzero((_bits(host) != _bits(want)).any(1))[0]
        assert len(bad) == 0, (kind, drag, bad[:8], host[bad[:2]], want[bad[:2]])
        d = Dev(mw, F)
        d.forces(o)
        assert _same(d.result(o)[1], want)


def test_one_coefficient_row_for_every_hull(mw):
    """Ocean.fleet_forces / step_fleet with a single row of coefficients (broadcast to the hulls), and with none: the single-hull calls
    with those coefficients"""
    o, span = _surface(mw, "fftmesh")
    F = _fleet(mw, span, seed=4)
    x, t, table = mw.pack_fleet(F.hulls)
    with o:
        for row in ([1000.0, 9.81, 20.0, 50.0, np.nan], None):
            G1 = Fleet(F.hulls, F.bodies, F.mass, o._fleet_coeffs(len(F.hulls), row))
            want, (wb, wr) = _single_forces(o, G1), _single_step(o, G1, 0.1, 4)
            assert _same(o.fleet_forces(x, t, table, F.bodies, coeffs=row), want) and (np.abs(want[:, 1]) > 1e3).any()
            b, r = o.step_fleet(x, t, table, F.bodies.copy(), F.mass, 0.1, substeps=4, coeffs=row, return_forces=True)
            assert _same(b, wb) and _same(r, wr)


# ---- 2. composition does not matter ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fftmesh", "periodic"])
def test_composition_does_not_matter(mw, kind):
    o, span = _surface(mw, kind)
    F = _fleet(mw, span, drag="each")
    with o:
        full = _fleet_forces(o, mw, F)
        fb, fr = _step_fleet(o, mw, F, 0.1, 4)
        for order in (list(range(len(F.hulls)))[::-1], list(range(0, len(F.hulls), 2)), [6]):
            sub, idx = F.pick(order)
            assert _same(_fleet_forces(o, mw, sub), full[idx]), order
            sb, sr = _step_fleet(o, mw, sub, 0.1, 4)
            assert _same(sb, fb[idx]) and _same(sr, fr[idx]), order


# ---- 3. stepping equals the single-hull calls -----------------------------------------------------------------------------
@pytest.mark.parametrize("drag", ["off", "each"])
@pytest.mark.parametrize("kind", ["fftmesh", "periodic"])
def test_stepping_equals_the_single_hull_calls(mw, plan, kind, drag):
    o, span = _surface(mw, kind)
    F = _fleet(mw, span, seed=6, drag=drag)
    with o:
        wb, wr = _single_step(o, F, 0.2, 8)
        assert np.isfinite(wb).all() and not np.array_equal(wb[:, 0:3], F.bodies[:, 0:3])
        b, r = _step_fleet(o, mw, F, 0.2, 8)  # wrench = NULL
        bad = np.nonzero((_bits(b) != _bits(wb)).any(1) | (_bits(r) != _bits(wr)).any(1))[0]
        assert len(bad) == 0, (plan, kind, drag, bad[:8])
        assert np.array_equal(b[:, [3, 11, 15]], F.bodies[:, [3, 11, 15]])
        d = Dev(mw, F)
        d.step(o, 0.2, 8)
        db, dr = d.result(o)
        assert _same(db, wb) and _same(dr, wr)


def test_stepping_on_the_renderer_equals_the_single_hull_calls(mw, plan):
    o, span = _surface(mw, "renderer")
    F = _fleet(mw, span, seed=8, drag="one")
    with o:
        wb, wr = _single_step(o, F, 0.1, 8)
        b, r = _step_fleet(o, mw, F, 0.1, 8)
        assert _same(b, wb) and _same(r, wr)


# ---- 4. wrench --------------------------------------------------------------------------------------------------------------
def test_wrench_holds_a_body_against_gravity_exactly(mw, plan):
    """m = 2, g = 9.81, Fy = 2 g far above the water: (2 g) / 2 - g is exactly 0 in float32, so v stays 0 and p keeps its bits"""
    x, t = H.box(1.0, 1.0, 1.0)
    big = H.grid_hull(12, 14, 2.5, 4.0, 1.0)  # 4 chunks: the per-substep kernels under the rule
    hulls = [(x, t, 2), big + (1,)]
    bodies = mw.pack_bodies([[1.0, 40.0, -2.0], [3.0, 55.5, 4.0], [-5.0, 61.25, 2.0]], H.random_quaternions(3, np.random.default_rng(1)))
    mass = mw.pack_mass(2.0, np.diag([1.0, 2.0, 3.0]))
    mass = np.repeat(mass, 3, 0)
    g = np.float32(9.81)
    cf = np.array([[RHO, g, 0, 0, 1]] * 2, np.float32)
    wrench = np.zeros((3, 8), np.float32)
    wrench[:, 1] = np.float32(2.0) * g
    F = Fleet(hulls, bodies, mass, cf)
    with _ocean(mw) as o:
        b, r = _step_fleet(o, mw, F, 0.4, 8, wrench=wrench)
        assert (r[:, :7] == 0).all()  # out reports the water row alone
        assert _same(b[:, 0:3], bodies[:, 0:3]) and (b[:, 8:11] == 0).all() and (b[:, 12:15] == 0).all()
        free, _ = _step_fleet(o, mw, F, 0.4, 8)
        assert (free[:, 9] < -3.0).all()


def test_wrench_torque_about_a_principal_axis(mw, plan):
    """a dry box under a torque about its y axis: w grows by h tau / I per substep; the state is body_ref.step fed F + Fw, tau + tw"""
    x, t = H.box(1.0, 2.0, 3.0)
    m, I = 300.0, B.box_inertia(300.0, 1.0, 2.0, 3.0)
    F = Fleet([(x, t, 1)], mw.pack_bodies([[2.0, 30.0, 1.0]]), mw.pack_mass(m, I), np.array([[RHO, G, 0, 0, 1]], np.float32))
    wrench = np.zeros((1, 8), np.float32)
    wrench[0, 1] = np.float32(m * G)  # carried, so that only the spin is left
    wrench[0, 5] = 40.0
    K, dt = 8, np.float32(0.16)
    h = float(dt / np.float32(K))
    with _ocean(mw) as o:
        b, r = _step_fleet(o, mw, F, dt, K, wrench=wrench)
    assert (r[0, :7] == 0).all()
    assert abs(b[0, 13] - K * h * 40.0 / I[1, 1]) <= 1e-5 * K * h * 40.0 / I[1, 1] and abs(b[0, 12]) <= 1e-6 and abs(b[0, 14]) <= 1e-6
    ref = F.bodies[0].astype(np.float64)
    row = np.zeros(8, np.float32)
    row[0:3] = r[0, 0:3] + wrench[0, 0:3]
    row[4:7] = r[0, 4:7] + wrench[0, 4:7]
    for _ in range(K):
        ref = B.step(ref, row, F.mass[0].astype(np.float64), G, h)
    for sl in (slice(0, 3), slice(4, 8), slice(8, 11), slice(12, 15)):  # the bound of test_first_substep_parity (tests/test_bodies_gpu.py)
        assert np.abs(b[0, sl] - ref[sl]).max() <= 2e-5 * (1 + np.abs(ref[sl]).max()), (sl, b[0, sl], ref[sl])


@pytest.mark.parametrize("kind", ["fftmesh", "periodic"])
def test_wrench_on_waves_and_a_nan_wrench_row(mw, plan, kind):
    o, span = _surface(mw, kind)
    F = _fleet(mw, span, seed=9, drag="each")
    rng = np.random.default_rng(10)
    wrench = (rng.standard_normal((len(F.bodies), 8)) * 3000.0).astype(np.float32)
    bad = wrench.copy()
    victims = [0, 40, len(F.bodies) - 1]  # the tetrahedron, a box, a body of the 4-chunk barge
    bad[victims[0], 1] = np.nan
    bad[victims[1], 4] = np.inf
    bad[victims[2], 6] = -np.inf
    with o:
        plain, _ = _step_fleet(o, mw, F, 0.2, 8)
        good, rg = _step_fleet(o, mw, F, 0.2, 8, wrench=wrench)
        assert np.isfinite(good).all() and (np.abs(good[:, 8:11] - plain[:, 8:11]).max(1) > 1e-3).all()
        d = Dev(mw, F, wrench=wrench)
        d.step(o, 0.2, 8)
        db, dr = d.result(o)
        assert _same(db, good) and _same(dr, rg)
        # the water row of the last substep is the row of hull forces at the state at its start: the wrench is not in it
        with pytest.raises(mw.MistralWaterError) as e:
            _step_fleet(o, mw, F, 0.2, 8, wrench=bad)
        assert e.value.status == mw.MW_EINVAL and b"wrench row of body 0 " in mw.lib().mw_last_error()
        d = Dev(mw, F, wrench=bad)
        d.step(o, 0.2, 8)
        db, dr = d.result(o)
        keep = np.setdiff1d(np.arange(len(F.bodies)), victims)
        assert np.isnan(dr[victims]).all() and _same(db[victims], F.bodies[victims])
        assert _same(db[keep], good[keep]) and _same(dr[keep], rg[keep])


# ---- 5. failures stay local -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["fftmesh", "periodic"])
def test_failures_stay_local(mw, plan, kind):
    o, span = _surface(mw, kind)
    F = _fleet(mw, span, seed=11, drag="one")
    n = len(F.bodies)
    with o:
        good, rg = _step_fleet(o, mw, F, 0.2, 8)
        fg = _fleet_forces(o, mw, F)
        # a non-finite pose: a NaN row and a frozen state for that body only
        P = Fleet(F.hulls, F.bodies.copy(), F.mass, F.coeffs)
        victims = [5, n - 2]
        P.bodies[5, 0] = np.nan
        P.bodies[n - 2, 4] = np.inf
        if kind == "fftmesh":
            # a body off the one footprint: the world-mode walk clamps to the mesh's edge (csrc/surface_query.h), so the single-hull
            # calls answer with the edge's water and the distance to it as the residual, not with NaN; the fleet row is that row
            P.bodies[70, 0] = 500.0
        keep = np.setdiff1d(np.arange(n), victims + [70])
        b, r = _step_fleet(o, mw, P, 0.2, 8)
        f = _fleet_forces(o, mw, P)
        assert np.isnan(r[victims]).all() and np.isnan(f[victims]).all() and _same(b[victims], P.bodies[victims])
        assert _same(b[keep], good[keep]) and _same(r[keep], rg[keep]) and _same(f[keep], fg[keep])
        x70, t70, _ = F.hulls[2]
        assert _same(f[70], o.hull_forces(x70, t70, P.bodies[70:71], **_kw(F.coeffs[2]))[0])
        s70 = o.step_bodies(x70, t70, P.bodies[70:71].copy(), F.mass[70:71], 0.2, substeps=8, return_forces=True, **_kw(F.coeffs[2]))
        assert _same(b[70], s70[0][0]) and _same(r[70], s70[1][0])
        assert (f[70, 7] > 400.0) == (kind == "fftmesh")
        # an invalid mass row: MW_EINVAL naming the body (host), a NaN row and an unchanged state (device)
        M = Fleet(F.hulls, F.bodies, F.mass.copy(), F.coeffs)
        M.mass[66, 0] = 0.0
        M.mass[2, 1:4] = [1.0, 1.0, -1.0]
        with pytest.raises(mw.MistralWaterError) as e:
            _step_fleet(o, mw, M, 0.2, 8)
        assert e.value.status == mw.MW_EINVAL and b"mass row of body 2 " in mw.lib().mw_last_error()
        d = Dev(mw, M)
        d.step(o, 0.2, 8)
        db, dr = d.result(o)
        keep = np.setdiff1d(np.arange(n), [2, 66])
        assert np.isnan(dr[[2, 66]]).all() and _same(db[[2, 66]], F.bodies[[2, 66]])
        assert _same(db[keep], good[keep]) and _same(dr[keep], rg[keep])
        # a triangle index outside [0, nverts_h): MW_EINVAL naming the hull (host), that hull's rows NaN and no other's (device)
        x, t, table = mw.pack_fleet(F.hulls)
        for h, value in ((2, 162), (6, -1)):
            tb = t.copy()
            tb[table[h, 2] + table[h, 3] - 1, 1] = value
            with pytest.raises(mw.MistralWaterError) as e:
                o.fleet_forces(x, tb, table, F.bodies, coeffs=F.coeffs)
            assert e.value.status == mw.MW_EINVAL and ("hull %d:" % h).encode() in mw.lib().mw_last_error()
            with pytest.raises(mw.MistralWaterError) as e:
                o.step_fleet(x, tb, table, F.bodies.copy(), F.mass, 0.2, coeffs=F.coeffs)
            assert e.value.status == mw.MW_EINVAL and ("hull %d:" % h).encode() in mw.lib().mw_last_error()
            rows = np.arange(n)[F.rows(h)]
            keep = np.setdiff1d(np.arange(n), rows)
            d = Dev(mw, F, tris=tb)
            d.forces(o)
            df = d.result(o)[1]
            assert np.isnan(df[rows]).all() and _same(df[keep], fg[keep])
            d = Dev(mw, F, tris=tb)
            d.step(o, 0.2, 8)
            db, dr = d.result(o)
            assert np.isnan(dr[rows]).all() and _same(db[rows], F.bodies[rows])
            assert _same(db[keep], good[keep]) and _same(dr[keep], rg[keep])


# ---- 6. argument and state rules ----------------------------------------------------------------------------------------
def test_argument_checks_leave_caller_arrays_untouched(mw):
    import torch
    L = mw.lib()
    F = _fleet(mw, 20.0, seed=12)
    x, t, table = mw.pack_fleet(F.hulls)
    n, nh = len(F.bodies), len(table)
    bodies, out = F.bodies.copy(), np.full((n, 8), 7.0, np.float32)
    cf = F.coeffs.copy()
    lim = 2 ** 31 - 256

    def tab(h, col, value, total=None):
        tb = table.copy()
        tb[h, col] = value
        return dict(hulls=tb, nb=int(tb[:, 4].sum()) if total is None else total)

    def coeff(h, col, value):
        c = cf.copy()
        c[h, col] = value
        return dict(cf=c)

    with _ocean(mw) as o:
        h = o._h

        def forces(hulls=table, nhulls=nh, nb=n, xx=_p(x), tt=_p(t), bb=_p(bodies), oo=_p(out), cf=cf, nv=len(x), nt=len(t), frame=-1, it=0,
                   **_):
            return L.mw_ocean_fleet_forces(h, frame, xx, nv, tt, nt, _p(hulls), nhulls, bb, nb, _p(cf), it, oo)

        def step(hulls=table, nhulls=nh, nb=n, xx=_p(x), tt=_p(t), bb=_p(bodies), mm=_p(F.mass), oo=_p(out), cf=cf, nv=len(x), nt=len(t),
                 frame=-1, it=0, sub=2, dt=0.1):
            return L.mw_ocean_step_fleet(h, frame, xx, nv, tt, nt, _p(hulls), nhulls, bb, mm, None, nb, _p(cf), C.c_float(dt), sub, it, oo)

        shared = [dict(nhulls=0), dict(nhulls=33), dict(nhulls=-1), dict(hulls=None), dict(cf=None), dict(hulls=None, nb=0), dict(cf=None, nb=0),
                  tab(1, 0, len(x) - 7), tab(1, 0, -1), tab(2, 2, len(t) - 319), tab(2, 2, -1), tab(0, 1, 2), tab(0, 3, 0), tab(1, 4, -1, total=n),
                  dict(nb=n + 1), dict(nb=-1), dict(nv=len(x) - 1), dict(nt=len(t) - 1),
                  tab(6, 4, 4_000_000), tab(7, 4, lim - n + 1), dict(xx=None), dict(tt=None), dict(bb=None),
                  coeff(0, 0, -1.0), coeff(3, 2, np.nan), coeff(7, 4, np.inf), dict(frame=0), dict(it=-1), dict(it=65)]
        for kw in shared:
            assert forces(**kw) == mw.MW_EINVAL, kw
            assert step(**kw) == mw.MW_EINVAL, kw
        assert forces(oo=None) == mw.MW_EINVAL
        for kw in (dict(sub=0), dict(sub=65), dict(dt=-0.1), dict(dt=float("nan")), dict(dt=float("inf")), dict(mm=None)):
            assert step(**kw) == mw.MW_EINVAL, kw
        assert np.array_equal(bodies, F.bodies) and (out == 7.0).all()
        # total_bodies == 0 does nothing; NULL per-body arrays are then allowed
        empty = table.copy()
        empty[:, 4] = 0
        assert forces(hulls=empty, nb=0, bb=None, oo=None, xx=None, tt=None) == mw.MW_OK
        assert step(hulls=empty, nb=0, bb=None, mm=None, oo=None) == mw.MW_OK
        assert (out == 7.0).all()
        assert step(oo=None) == mw.MW_OK and forces() == mw.MW_OK  # these two write: bodies moves on, out is filled
        assert not np.array_equal(bodies, F.bodies) and np.isfinite(out).all()
        snap = bodies.copy()
        out[:] = 7.0
        # the device forms: misalignment
        buf = torch.zeros(1 << 16, dtype=torch.float32, device="cuda")
        base = buf.data_ptr()
        one = np.array([[0, 8, 0, 12, 1]], np.int32)
        for off_b, off_m, off_w, off_o in ((4, 0, 0, 0), (0, 8, 0, 0), (0, 0, 4, 0), (0, 0, 0, 8)):
            s = L.mw_ocean_step_fleet_device(h, -1, C.c_void_p(base + 8192), 8, C.c_void_p(base + 12288), 12, _p(one), 1, C.c_void_p(base + off_b),
                                             C.c_void_p(base + 1024 + off_m), C.c_void_p(base + 2048 + off_w), 1, _p(cf), C.c_float(0.1), 1, 0,
                                             C.c_void_p(base + 4096 + off_o))
            assert s == mw.MW_EINVAL
        for off_b, off_o in ((4, 0), (0, 8)):
            s = L.mw_ocean_fleet_forces_device(h, -1, C.c_void_p(base + 8192), 8, C.c_void_p(base + 12288), 12, _p(one), 1,
                                               C.c_void_p(base + off_b), 1, _p(cf), 0, C.c_void_p(base + 4096 + off_o))
            assert s == mw.MW_EINVAL
    with mw.Ocean(resolution=16, unit_width=1.0, length=27.155 * 2, wind=(14.45, 12.0), amplitude=0.41, choppiness=1.5, mult=1.5, seed=1,
                  semantics=mw.MW_SEM_OCEANRENDERER, device=0, ntiles=2) as r:
        h = r._h
        assert forces() == mw.MW_EINVAL and step() == mw.MW_EINVAL and b"batched" in L.mw_last_error()
    assert np.array_equal(bodies, snap) and (out == 7.0).all()


def test_frame_and_state_rules(mw, oracle):
    F = _fleet(mw, 20.0, seed=13, drag="off")
    D = _fleet(mw, 20.0, seed=13, drag="one")
    p = workloads.fftmesh_params(64)
    with _ocean(mw, frame=False) as o:
        for fn in (lambda: _fleet_forces(o, mw, F), lambda: _step_fleet(o, mw, F, 0.1, 2)):
            with pytest.raises(mw.MistralWaterError) as e:
                fn()
            assert e.value.status == mw.MW_ESTATE  # no frame yet
        o.evaluate(1.0)
        _fleet_forces(o, mw, D)
        h0, h0c = oracle.generate_spectrum(p, 3)
        o.set_spectrum(h0, h0c)
        _fleet_forces(o, mw, F)  # no hull has drag: the surface query's rules
        _step_fleet(o, mw, F, 0.1, 2)
        for fn in (lambda: _fleet_forces(o, mw, D), lambda: _step_fleet(o, mw, D, 0.1, 2)):
            with pytest.raises(mw.MistralWaterError) as e:
                fn()
            assert e.value.status == mw.MW_ESTATE  # one hull has drag: the velocity query's
        o.evaluate(1.5)
        _fleet_forces(o, mw, D)


# ---- 7. no state changes ------------------------------------------------------------------------------------------------
def test_fleet_calls_change_no_state(mw):
    F = _fleet(mw, 20.0, seed=14, drag="each")
    x, t, nb = F.hulls[2]
    s = F.rows(2)
    xz = np.ascontiguousarray(np.random.default_rng(1).uniform(-25, 25, (50, 2)), np.float32)

    def run(with_fleet):
        out = []
        with _ocean(mw, frame=False) as o:
            for k in range(3):
                v, n, c = o.update(0.03)
                if with_fleet:
                    _fleet_forces(o, mw, F)
                    _step_fleet(o, mw, F, 0.1, 4)
                out += [v, n, c, np.float32(o.timer), o.query_surface(xz, mode="world"), o.query_velocity(xz, mode="world"),
                        o.hull_forces(x, t, F.bodies[s], **_kw(F.coeffs[2])),
                        o.step_bodies(x, t, F.bodies[s].copy(), F.mass[s], 0.1, substeps=4, **_kw(F.coeffs[2]))]
        return out

    a, b = run(False), run(True)
    assert all(_same(np.atleast_1d(p), np.atleast_1d(q)) for p, q in zip(a, b))
    with _renderer(mw) as r:
        ph = r.get_phase()
        R = _fleet(mw, 3.0, seed=14, drag="one")
        _fleet_forces(r, mw, R)
        _step_fleet(r, mw, R, 0.1, 4)
        assert np.array_equal(r.get_phase(), ph)


@pytest.mark.parametrize("kind", ["fftmesh", "periodic"])
def test_two_device_calls_back_to_back(mw, kind):
    """two device-form calls with different tables enqueued without a synchronise in between: each reads its own table"""
    o, span = _surface(mw, kind)
    F = _fleet(mw, span, seed=15, drag="each")
    A, ia = F.pick([6, 1, 0, 7, 2])
    Bf, ib = F.pick([3, 5, 4])
    with o:
        fa, fb = _fleet_forces(o, mw, A), _fleet_forces(o, mw, Bf)
        sa, sb = _step_fleet(o, mw, A, 0.1, 4), _step_fleet(o, mw, Bf, 0.1, 4)
        da, db = Dev(mw, A), Dev(mw, Bf)
        da.forces(o)
        db.forces(o)
        assert _same(da.result(o)[1], fa) and _same(db.result(o)[1], fb)
        da.step(o, 0.1, 4)
        db.step(o, 0.1, 4)
        ra, rb = da.result(o), db.result(o)
        assert _same(ra[0], sa[0]) and _same(ra[1], sa[1]) and _same(rb[0], sb[0]) and _same(rb[1], sb[1])
