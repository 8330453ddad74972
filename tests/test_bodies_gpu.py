"""GPU tier of the floating bodies (mw_ocean_step_bodies / _device, include/mistral_water.h) through the C ABI: free fall, equilibrium,
heave period, damping, roll and spin on flat water (a zero spectrum); parity of the first substep with mw_ocean_hull_forces_device and
tests/body_ref.py on waves; composition of substeps; bitwise reproducibility (host vs device form, a body alone vs in a batch of 1000,
the two plans of switch MW_BODIES_PLAN); the NaN, mass-row, frame and state rules; a soak on waves."""
import ctypes as C

import numpy as np
import pytest

import body_ref as B
import hull_ref as H
import workloads

pytestmark = pytest.mark.gpu
RHO, G = 1000.0, 9.81


def _ocean(mw, N=256, choppiness=0.46, seed=1):
    p = workloads.fftmesh_params(N, choppiness=choppiness)
    return mw.Ocean(resolution=p.N, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                    choppiness=p.choppiness, gravity=p.gravity, seed=seed, device=0)


def _renderer(mw, res, seed=1):
    return mw.Ocean(resolution=res, unit_width=1.0, length=27.155 * res / 8, wind=(14.45, 12.0), amplitude=0.41, choppiness=1.5,
                    mult=1.5, seed=seed, semantics=mw.MW_SEM_OCEANRENDERER, device=0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _flat(mw):
    """a 256^2 FFTMesh with a zero spectrum: every vertex at its rest position, height 0 (footprint +-128)"""
    o = _ocean(mw)
    z = np.zeros((o.N, o.N, 2), np.float32)
    o.set_spectrum(z, z)
    o.evaluate(1.0)
    return o


@pytest.fixture(params=[0, 1], ids=["per_substep", "one_launch"])
def plan(request, mw):
    old = mw.get_switch("MW_BODIES_PLAN")
    mw.set_switch("MW_BODIES_PLAN", request.param)
    yield request.param
    mw.set_switch("MW_BODIES_PLAN", old)


def _box_body(mw, w, h, l, density):
    x, t = H.box(w, h, l)
    m = density * w * h * l
    return x, t, mw.pack_mass(m, B.box_inertia(m, w, h, l))


def _tilt(body):
    """angle (degrees) between the body's y axis and the world's"""
    R = H.rotation(body[4:8])[0]
    return float(np.degrees(np.arccos(np.clip(R[1, 1], -1, 1))))


def test_free_fall_closed_form(mw, plan):
    x, t, mass = _box_body(mw, 1.0, 1.0, 1.0, 500.0)
    body = mw.pack_bodies([[3.0, 10.0, -2.0]], velocity=[[1.0, 2.0, 0.5]])
    K, dt = 8, np.float32(0.4)
    with _flat(mw) as o:
        b, rows = o.step_bodies(x, t, body.copy(), mass, dt, substeps=K, return_forces=True)
    h = float(np.float32(dt) / np.float32(K))
    assert (rows[0, :7] == 0).all()
    v = np.array([1.0, 2.0 - K * h * G, 0.5])
    p = np.array([3.0, 10.0, -2.0]) + K * h * np.array([1.0, 2.0, 0.5]) - np.array([0, h * h * G * K * (K + 1) / 2, 0])
    assert np.abs(b[0, 8:11] - v).max() <= 2e-6 * 20 and np.abs(b[0, 0:3] - p).max() <= 2e-6 * 20
    assert np.array_equal(b[0, 4:8], body[0, 4:8]) and (b[0, 12:15] == 0).all()


def test_equilibrium_stays(mw, plan):
    """a box of half the water's density released at its draft (centre at the waterline) stays there for 1000 substeps"""
    x, t, mass = _box_body(mw, 2.0, 1.0, 3.0, 500.0)
    b = mw.pack_bodies([[5.0, 0.0, -7.0]])
    with _flat(mw) as o:
        for _ in range(20):
            o.step_bodies(x, t, b, mass, 0.5, substeps=50)
    assert abs(b[0, 1]) < 1e-3 and np.abs(b[0, 8:11]).max() < 1e-3 and np.abs(b[0, 12:15]).max() < 1e-3
    assert abs(b[0, 0] - 5.0) < 1e-3 and abs(b[0, 2] + 7.0) < 1e-3 and _tilt(b[0]) < 0.01


def test_heave_period(mw):
    """undamped, released 0.1 h high: the period from zero crossings over 3 periods is 2 pi sqrt(m / (rho g A_wp)) to 1 %"""
    x, t, mass = _box_body(mw, 2.0, 1.0, 3.0, 500.0)
    T = 2 * np.pi * np.sqrt(float(mass[0, 0]) / (RHO * G * 6.0))
    b = mw.pack_bodies([[0.0, 0.1, 0.0]])
    dt, K = 0.008, 4
    ys, ts = [0.1], [0.0]
    with _flat(mw) as o:
        while ts[-1] < 3.3 * T:
            o.step_bodies(x, t, b, mass, dt, substeps=K)
            ys.append(float(b[0, 1]))
            ts.append(ts[-1] + dt)
    ys, ts = np.array(ys), np.array(ts)
    k = np.nonzero((ys[:-1] > 0) & (ys[1:] <= 0))[0]  # downward crossings
    tc = ts[k] + (ts[k + 1] - ts[k]) * ys[k] / (ys[k] - ys[k + 1])
    assert len(tc) >= 3
    period = (tc[-1] - tc[0]) / (len(tc) - 1)
    assert abs(period - T) <= 0.01 * T, (period, T)
    assert 0.09 <= ys.max() <= 0.101 and -0.101 <= ys.min() <= -0.09


def test_linear_drag_settles(mw):
    x, t, mass = _box_body(mw, 2.0, 1.0, 3.0, 500.0)
    b = mw.pack_bodies([[0.0, 0.1, 0.0]])
    with _flat(mw) as o:
        for _ in range(80):
            o.step_bodies(x, t, b, mass, 0.128, substeps=64, linear_drag=500.0)
    assert abs(b[0, 1]) < 1e-3 and np.abs(b[0, 8:15]).max() < 1e-3


def test_roll_returns_upright(mw):
    """a stable wide box (GM > 0) tilted 5 degrees: upright again with drag, within +-5.5 degrees without"""
    x, t, mass = _box_body(mw, 4.0, 1.0, 4.0, 500.0)
    q = [0.0, 0.0, np.sin(np.radians(2.5)), np.cos(np.radians(2.5))]
    free = mw.pack_bodies([[0.0, 0.0, 0.0]], [q])
    damped = free.copy()
    worst = 0.0
    with _flat(mw) as o:
        for _ in range(80):
            o.step_bodies(x, t, free, mass, 0.064, substeps=32)
            o.step_bodies(x, t, damped, mass, 0.064, substeps=32, linear_drag=1000.0)
            worst = max(worst, _tilt(free[0]))
    assert 4.5 <= worst <= 5.5, worst
    assert _tilt(damped[0]) < 0.5 and np.isfinite(damped).all()


def test_spin_about_principal_axis(mw, plan):
    x, t, mass = _box_body(mw, 1.0, 2.0, 3.0, 300.0)
    b = mw.pack_bodies([[0.0, 20.0, 0.0]], angular_velocity=[[0.0, 2.5, 0.0]])
    K, dt = 16, np.float32(0.32)
    with _flat(mw) as o:
        o.step_bodies(x, t, b, mass, dt, substeps=K)
    h = float(np.float32(dt) / np.float32(K))
    angle = 2 * np.arctan2(np.linalg.norm(b[0, 4:7]), b[0, 7])
    assert abs(angle - 2 * K * np.arctan(h * 2.5 / 2)) <= 2e-6 * K and abs(b[0, 13] - 2.5) <= 1e-5
    assert abs(b[0, 4]) <= 1e-6 and abs(b[0, 6]) <= 1e-6


def _fleet(mw, rng, n, span, hull, tris, density=600.0, moving=True):
    m, c, I = mw.hull_mass_properties(hull, tris, density)
    p = np.stack([rng.uniform(-span, span, n), rng.uniform(-0.5, 0.5, n), rng.uniform(-span, span, n)], 1)
    v = rng.standard_normal((n, 3)) if moving else None
    w = rng.standard_normal((n, 3)) if moving else None
    return mw.pack_bodies(p, H.random_quaternions(n, rng), v, w), mw.pack_mass(np.full(n, m), I), np.asarray(hull - c, np.float32)


def _device(o, hull, tris, bodies, mass, dt, substeps, **kw):
    import torch
    d_h, d_t = torch.from_numpy(np.ascontiguousarray(hull)).cuda(), torch.from_numpy(np.ascontiguousarray(tris)).cuda()
    d_b, d_m = torch.from_numpy(bodies.copy()).cuda(), torch.from_numpy(np.ascontiguousarray(mass)).cuda()
    d_o = torch.zeros((len(bodies), 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    o.step_bodies_device(d_h.data_ptr(), len(hull), d_t.data_ptr(), len(tris), d_b.data_ptr(), d_m.data_ptr(), len(bodies), dt,
                         substeps, d_o.data_ptr(), **kw)
    o.synchronize()
    return d_b.cpu().numpy(), d_o.cpu().numpy()


@pytest.mark.parametrize("sem", ["fftmesh", "renderer"])
@pytest.mark.parametrize("drag", [False, True])
def test_first_substep_parity(mw, plan, sem, drag):
    """substeps = 1: the out row is hull_forces_device's bit for bit, and the new state is body_ref's step applied to that row"""
    import torch
    rng = np.random.default_rng(5)
    if sem == "fftmesh":
        o = _ocean(mw, 256, choppiness=1.0)
        o.evaluate(2.3)
        span = 80.0
    else:
        o = _renderer(mw, 64)
        for dt in (0.3, 0.4):
            o.generate_texture(dt)
        span = 20.0
    kw = dict(linear_drag=30.0, quadratic_drag=60.0) if drag else {}
    with o:
        for hull0, tris in (H.icosphere(1.5), H.grid_hull(6, 10, 3.0, 5.0, 0.8)):
            bodies, mass, hull = _fleet(mw, rng, 24, span, hull0, tris)
            d_h, d_t, d_b = torch.from_numpy(hull).cuda(), torch.from_numpy(tris).cuda(), torch.from_numpy(bodies).cuda()
            d_o = torch.empty((len(bodies), 8), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            o.hull_forces_device(d_h.data_ptr(), len(hull), d_t.data_ptr(), len(tris), d_b.data_ptr(), len(bodies), d_o.data_ptr(), **kw)
            o.synchronize()
            want = d_o.cpu().numpy()
            dt = 1.0 / 60
            b, rows = _device(o, hull, tris, bodies, mass, dt, 1, **kw)
            assert np.array_equal(_bits(rows), _bits(want))
            assert np.isfinite(want).all() and (want[:, 3] > 0).any()
            for k in range(len(bodies)):
                ref = B.step(bodies[k], want[k], mass[k].astype(np.float64), G, float(np.float32(dt)))
                for sl in (slice(0, 3), slice(4, 8), slice(8, 11), slice(12, 15)):
                    assert np.abs(b[k, sl] - ref[sl]).max() <= 2e-5 * (1 + np.abs(ref[sl]).max()), (k, sl, b[k, sl], ref[sl])
                assert np.array_equal(b[k, [3, 11, 15]], bodies[k, [3, 11, 15]])


def test_composition_of_substeps(mw, plan):
    """one call with K substeps = K calls with dt / K (f32), bit for bit; out = the last call's row"""
    rng = np.random.default_rng(8)
    bodies, mass, hull = _fleet(mw, rng, 40, 80.0, *H.icosphere(1.2))
    tris = H.icosphere(1.2)[1]
    K, dt = 8, np.float32(0.25)
    with _ocean(mw, 256, choppiness=1.0) as o:
        o.evaluate(3.1)
        for kw in ({}, dict(linear_drag=20.0, quadratic_drag=40.0)):
            one, r1 = o.step_bodies(hull, tris, bodies.copy(), mass, dt, substeps=K, return_forces=True, **kw)
            many = bodies.copy()
            for _ in range(K):
                many, rk = o.step_bodies(hull, tris, many, mass, float(dt / np.float32(K)), return_forces=True, **kw)
            assert np.array_equal(_bits(one), _bits(many)) and np.array_equal(_bits(r1), _bits(rk))
            assert not np.array_equal(one, bodies)


def test_reproducible_host_device_batch(mw):
    rng = np.random.default_rng(3)
    hull0, tris = H.icosphere(2.0)
    bodies, mass, hull = _fleet(mw, rng, 1000, 110.0, hull0, tris)
    with _ocean(mw, 256, choppiness=1.2) as o:
        o.evaluate(4.0)
        for kw in ({}, dict(linear_drag=30.0, quadratic_drag=70.0)):
            a, ra = o.step_bodies(hull, tris, bodies.copy(), mass, 0.2, substeps=4, return_forces=True, **kw)
            assert np.isfinite(a).all() and (ra[:, 3] > 0).any()
            b, rb = _device(o, hull, tris, bodies, mass, 0.2, 4, **kw)
            assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(ra), _bits(rb))
            for k in (0, 1, 517, 999):
                one, r1 = o.step_bodies(hull, tris, bodies[k:k + 1].copy(), mass[k:k + 1], 0.2, substeps=4, return_forces=True, **kw)
                assert np.array_equal(_bits(one[0]), _bits(a[k])) and np.array_equal(_bits(r1[0]), _bits(ra[k])), k


def _run_plan(mw, value, fn):
    old = mw.get_switch("MW_BODIES_PLAN")
    mw.set_switch("MW_BODIES_PLAN", value)
    try:
        return fn()
    finally:
        mw.set_switch("MW_BODIES_PLAN", old)


@pytest.mark.parametrize("hull_name", ["icosphere", "grid_hull"])
def test_plans_give_the_same_bits(mw, hull_name):
    """MW_BODIES_PLAN 0 vs 1 with 8 substeps, drag off and on, including a body with a huge angular velocity.  Drag off, its first row
    is finite (w is not read) and the first substep makes w and q non-finite, so its row holds a NaN from the second substep on and the
    state stays non-finite.  Drag on, w already enters the first substep's drag: that row holds a NaN and the body keeps its bits."""
    rng = np.random.default_rng(12)
    hull0, tris = H.icosphere(1.5) if hull_name == "icosphere" else H.grid_hull(25, 50, 6.0, 20.0, 2.0)
    n = 64 if hull_name == "icosphere" else 8
    bodies, mass, hull = _fleet(mw, rng, n, 90.0, hull0, tris)
    bodies[0, 12:15] = [1e30, 2e30, -1e30]
    with _ocean(mw, 256, choppiness=1.0) as o:
        o.evaluate(2.7)
        for kw in ({}, dict(linear_drag=25.0, quadratic_drag=50.0)):
            run = lambda: o.step_bodies(hull, tris, bodies.copy(), mass, 0.4, substeps=8, return_forces=True, **kw)  # noqa: E731
            a, ra = _run_plan(mw, 0, run)
            b, rb = _run_plan(mw, 1, run)
            assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(ra), _bits(rb))
            assert np.isnan(ra[0]).any()  # drag on, only F and tau: the area and residual stay finite
            if kw:
                assert np.array_equal(_bits(a[0]), _bits(bodies[0]))
            else:
                assert not np.isfinite(a[0]).all()
            assert np.isfinite(ra[1:]).all() and np.isfinite(a[1:]).all()


def test_nan_rows_freeze_the_body(mw, plan):
    """a non-finite pose from the start: bits unchanged, row NaN; a pose turning non-finite mid-call: the state at the start of the
    failing substep, bit for bit"""
    hull0, tris = H.icosphere(1.0)
    bodies, mass, hull = _fleet(mw, np.random.default_rng(4), 3, 20.0, hull0, tris)
    bodies[1, 0] = np.nan
    bodies[2, 12:15] = [1e30, 2e30, -1e30]
    with _ocean(mw, 256) as o:
        o.evaluate(1.5)
        a, ra = o.step_bodies(hull, tris, bodies.copy(), mass, 0.4, substeps=8, return_forces=True)
        assert np.array_equal(_bits(a[1]), _bits(bodies[1])) and np.isnan(ra[1]).all()
        assert np.isfinite(ra[0]).all() and np.isnan(ra[2]).all()
        b = bodies[2:3].copy()
        for _ in range(8):  # one substep per call until the row is NaN: the state there is the frozen one
            prev = b.copy()
            b, rb = o.step_bodies(hull, tris, b, mass[2:3], float(np.float32(0.4) / np.float32(8)), return_forces=True)
            if np.isnan(rb).any():
                assert np.array_equal(_bits(b), _bits(prev))
                break
        else:
            pytest.fail("the pose never turned non-finite")
        assert np.array_equal(_bits(a[2]), _bits(b[0]))


def test_invalid_mass_rows(mw, plan):
    hull0, tris = H.icosphere(1.0)
    bodies, mass, hull = _fleet(mw, np.random.default_rng(6), 5, 20.0, hull0, tris)
    bad = mass.copy()
    bad[3, 0] = 0.0
    bad[1, 1:4] = [1.0, 1.0, -1.0]  # not positive definite
    with _ocean(mw, 256) as o:
        o.evaluate(1.5)
        with pytest.raises(mw.MistralWaterError) as e:
            o.step_bodies(hull, tris, bodies.copy(), bad, 0.1, substeps=2)
        assert e.value.status == mw.MW_EINVAL and b"body 1" in mw.lib().mw_last_error()
        good, rg = o.step_bodies(hull, tris, bodies.copy(), mass, 0.1, substeps=2, return_forces=True)
        b, rb = _device(o, hull, tris, bodies, bad, 0.1, 2)
        for k in (1, 3):
            assert np.isnan(rb[k]).all() and np.array_equal(_bits(b[k]), _bits(bodies[k]))
        for k in (0, 2, 4):
            assert np.array_equal(_bits(b[k]), _bits(good[k])) and np.array_equal(_bits(rb[k]), _bits(rg[k]))


def test_argument_checks(mw):
    L = mw.lib()
    _p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    x, t, mass = _box_body(mw, 1.0, 1.0, 1.0, 500.0)
    body = mw.pack_bodies([[0.0, 0.0, 0.0]])
    cf = np.array([RHO, G, 0, 0, 1], np.float32)
    out = np.zeros((1, 8), np.float32)
    with _ocean(mw, 64) as o:
        o.evaluate(1.0)
        h = o._h

        def call(sub=1, dt=0.1, mm=_p(mass), oo=_p(out), nb=1, frame=-1):
            return L.mw_ocean_step_bodies(h, frame, _p(x), 8, _p(t), 12, _p(body), mm, nb, _p(cf), C.c_float(dt), sub, 0, oo)
        assert call() == mw.MW_OK and call(oo=None) == mw.MW_OK
        for kw in (dict(sub=0), dict(sub=65), dict(dt=-0.1), dict(dt=float("nan")), dict(dt=float("inf")), dict(mm=None),
                   dict(frame=0), dict(nb=-1)):
            assert call(**kw) == mw.MW_EINVAL, kw
        assert call(sub=64) == mw.MW_OK and call(dt=0.0) == mw.MW_OK
        import torch
        buf = torch.zeros(64 * 40, dtype=torch.float32, device="cuda")
        base = buf.data_ptr()
        for off_b, off_m, off_o in ((4, 0, 0), (0, 8, 0), (0, 0, 4)):
            s = L.mw_ocean_step_bodies_device(h, -1, C.c_void_p(base + 4096), 8, C.c_void_p(base + 5120), 12, C.c_void_p(base + off_b),
                                              C.c_void_p(base + 1024 + off_m), 1, _p(cf), C.c_float(0.1), 1, 0,
                                              C.c_void_p(base + 2048 + off_o))
            assert s == mw.MW_EINVAL


def test_frame_and_state_rules(mw, oracle):
    x, t, mass = _box_body(mw, 1.0, 1.0, 1.0, 500.0)
    body = mw.pack_bodies([[0.3, 0.0, -0.2]])
    p = workloads.fftmesh_params(64)
    with _ocean(mw, 64) as o:
        with pytest.raises(mw.MistralWaterError) as e:
            o.step_bodies(x, t, body.copy(), mass, 0.1)
        assert e.value.status == mw.MW_ESTATE  # no frame yet
        o.evaluate(1.0)
        o.step_bodies(x, t, body.copy(), mass, 0.1, linear_drag=1.0)
        h0, h0c = oracle.generate_spectrum(p, 3)
        o.set_spectrum(h0, h0c)
        o.step_bodies(x, t, body.copy(), mass, 0.1)  # drag off: the surface query's rules
        with pytest.raises(mw.MistralWaterError) as e:
            o.step_bodies(x, t, body.copy(), mass, 0.1, quadratic_drag=1.0)
        assert e.value.status == mw.MW_ESTATE
    with _renderer(mw, 32) as r:
        r.generate_texture_steps([0.05, 0.1, 0.07])
        rb = mw.pack_bodies([[1.0, 0.0, 2.0], [-3.0, 0.2, 1.0]])
        m2 = np.repeat(mass, 2, 0)
        outs = [r.step_bodies(x, t, rb.copy(), m2, 0.05, frame=k) for k in range(3)]
        assert not np.array_equal(outs[0], outs[2])
        r.step_bodies(x, t, rb.copy(), m2, 0.05, frame=2, linear_drag=3.0)
        with pytest.raises(mw.MistralWaterError) as e:
            r.step_bodies(x, t, rb.copy(), m2, 0.05, frame=1, linear_drag=3.0)
        assert e.value.status == mw.MW_EINVAL


def test_step_bodies_change_no_state(mw):
    x, t, mass = _box_body(mw, 1.5, 1.0, 2.0, 400.0)
    rng = np.random.default_rng(1)
    bodies = mw.pack_bodies(rng.uniform(-60, 60, (8, 3)) * [1, 0, 1])
    m8 = np.repeat(mass, 8, 0)
    xz = np.ascontiguousarray(rng.uniform(-100, 100, (50, 2)), np.float32)

    def run(with_bodies):
        out = []
        with _ocean(mw, 256) as o:
            for k in range(3):
                v, n, c = o.update(0.03)
                if with_bodies:
                    o.step_bodies(x, t, bodies.copy(), m8, 0.1, substeps=4)
                    o.step_bodies(x, t, bodies.copy(), m8, 0.1, substeps=4, linear_drag=5.0, quadratic_drag=5.0)
                out += [v, n, c, np.float32(o.timer), o.query_surface(xz, mode="world"), o.query_velocity(xz, mode="world")]
        return out

    a, b = run(False), run(True)
    assert all(np.array_equal(_bits(np.atleast_1d(p)), _bits(np.atleast_1d(q))) for p, q in zip(a, b))


def test_soak_fleet_on_waves(mw):
    """64 icosphere buoys for 8 frames x 8 substeps on waves, the ocean advanced between calls: finite and near the surface"""
    rng = np.random.default_rng(9)
    hull0, tris = H.icosphere(1.0)
    bodies, mass, hull = _fleet(mw, rng, 64, 60.0, hull0, tris, density=500.0, moving=False)
    bodies[:, 1] = 0.0
    with _ocean(mw, 256, choppiness=1.0) as o:
        o.evaluate(2.0)
        for _ in range(8):
            o.update(1.0 / 30)
            o.step_bodies(hull, tris, bodies, mass, 1.0 / 30, substeps=8, linear_drag=50.0, quadratic_drag=50.0)
        assert np.isfinite(bodies).all()
        eta = o.query_surface(np.ascontiguousarray(bodies[:, [0, 2]]), mode="world")[:, 1]
    assert np.abs(bodies[:, 1] - eta).max() < 3.0
    assert np.abs(np.linalg.norm(bodies[:, 4:8], axis=1) - 1).max() < 1e-5
