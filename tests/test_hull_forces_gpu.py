"""GPU tier of the hull forces (mw_ocean_hull_forces / _device, include/mistral_water.h) through the C ABI: Archimedes on flat water on
every surface path, parity on waves with the f64 reference (tests/hull_ref.py) fed the library's own query answers, bitwise
reproducibility (repeated calls, host vs device form, a body alone vs in a batch of 1000), no state change, the frame and state rules,
and NaN rows for bad device indices."""
import numpy as np
import pytest

import hull_ref as H
import surface_ref as S
import workloads

pytestmark = pytest.mark.gpu
RHO, G = 1000.0, 9.81


def _ocean(mw, p, seed=1):
    return mw.Ocean(resolution=p.N, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                    choppiness=p.choppiness, gravity=p.gravity, seed=seed, device=0)


def _renderer(mw, res, choppiness=1.5, seed=1):
    return mw.Ocean(resolution=res, unit_width=1.0, length=27.155 * res / 8, wind=(14.45, 12.0), amplitude=0.41, choppiness=choppiness,
                    mult=1.5, seed=seed, semantics=mw.MW_SEM_OCEANRENDERER, device=0)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _flatten(o, renderer=False):
    """zero spectrum: every vertex at its rest position, height 0"""
    z = np.zeros((o.N, o.N, 2), np.float32)
    o.set_spectrum(z, z)
    if renderer:
        o.generate_texture(0.02)
    else:
        o.evaluate(1.0)


def _bodies(mw, n, rng, span, dy=(-0.6, 0.6), rotate=True, moving=True):
    p = np.stack([rng.uniform(-span, span, n), rng.uniform(*dy, n), rng.uniform(-span, span, n)], 1)
    q = H.random_quaternions(n, rng) if rotate else None
    v = rng.standard_normal((n, 3)) if moving else None
    w = rng.standard_normal((n, 3)) if moving else None
    return mw.pack_bodies(p, q, v, w)


def _archimedes(rows, bodies, hull, tris):
    x = H.transform(bodies, hull)
    for b in range(len(bodies)):
        V, cB = H.submerged(x[b], tris)
        F = np.array([0.0, RHO * G * V, 0.0])
        tau = np.cross(cB - bodies[b, 0:3].astype(np.float64), F)
        scale = RHO * G * H.volume(x[b], tris)  # the hull's full buoyancy bounds every contribution's sum
        assert np.abs(rows[b, 0:3] - F).max() <= 2e-5 * scale, (b, rows[b], F)
        assert np.abs(rows[b, 4:7] - tau).max() <= 2e-5 * scale * (1 + np.abs(hull).max()), (b, rows[b], tau)
        assert rows[b, 7] <= 1e-4


SURFACES = ["fft256", "fft1024", "czt12", "renderer128"]


def _flat_surface(mw, name):
    if name == "renderer128":
        o = _renderer(mw, 128)
        _flatten(o, renderer=True)
        return o, 40.0
    N = {"fft256": 256, "fft1024": 1024, "czt12": 12}[name]
    p = workloads.shipped_fftmesh_scene() if N == 12 else workloads.fftmesh_params(N)
    o = _ocean(mw, p)
    _flatten(o)
    return o, (3.0 if N == 12 else 60.0)


@pytest.mark.parametrize("name", SURFACES)
def test_archimedes_on_flat_water(mw, name):
    o, span = _flat_surface(mw, name)
    rng = np.random.default_rng(len(name))
    with o:
        for hull, tris in (H.box(2.0, 0.8, 1.5), H.icosphere(1.0)):
            bodies = _bodies(mw, 16, rng, span, moving=False)
            rows = o.hull_forces(hull, tris, bodies)
            _archimedes(rows, bodies, hull, tris)
        # the axis-aligned box: V = w l draft exactly
        hull, tris = H.box(2.0, 1.0, 4.0)
        rows = o.hull_forces(hull, tris, mw.pack_bodies([[0.5, 0.25, -0.5]]))
        assert abs(rows[0, 1] - RHO * G * 2 * 4 * 0.25) <= 1e-5 * RHO * G * 2
        assert abs(rows[0, 3] - (8 + 12 * 0.25)) <= 1e-5 * 11
        # fully submerged: rho g V_mesh; fully dry: exact zeros
        hull, tris = H.icosphere(0.8)
        rows = o.hull_forces(hull, tris, mw.pack_bodies([[0, -3.0, 0], [0, 2.0, 0]]), linear_drag=1.0, quadratic_drag=1.0)
        assert abs(rows[0, 1] - RHO * G * H.volume(hull, tris)) <= 1e-5 * RHO * G * H.volume(hull, tris)
        assert (rows[1, :7] == 0).all() and not np.signbit(rows[1, :7]).any()


def _water_at(o, x, frame=-1, iterations=0, drag=False, vscale=1.0):
    """the library's own answers at instance vertices x [n, V, 3] (float32): depth, water velocity, residual"""
    xz = np.ascontiguousarray(x.reshape(-1, 3)[:, [0, 2]], np.float32)
    qs = o.query_surface(xz, mode="world", frame=frame, iterations=iterations)
    d = (qs[:, 1] - x.reshape(-1, 3)[:, 1]).reshape(x.shape[:2])
    u = np.zeros(x.shape, np.float32)
    if drag:
        u = (o.query_velocity(xz, mode="world", frame=frame, iterations=iterations)[:, :3] * np.float32(vscale)).reshape(x.shape)
    return d, u, qs[:, 7].reshape(x.shape[:2])


def _parity(mw, o, hull, tris, bodies, lin, quad, vscale, frame=-1, identity=False):
    rows = o.hull_forces(hull, tris, bodies, linear_drag=lin, quadratic_drag=quad, velocity_scale=vscale, frame=frame)
    x = H.transform(bodies, hull).astype(np.float32)
    d, u, res = _water_at(o, x, frame=frame, drag=lin > 0 or quad > 0, vscale=vscale)
    if identity:  # x = p + h exactly: the same located points, so the same residuals, bit for bit
        assert np.array_equal(_bits(rows[:, 7]), _bits(res.max(1)))
    for b in range(len(bodies)):
        ref = H.forces(x[b], d[b], u[b], tris, bodies[b], RHO, G, lin, quad)
        scale = RHO * G * H.volume(x[b].astype(np.float64), tris) + (lin + quad) * 4 * np.abs(ref[3]) * 10
        assert np.isfinite(rows[b]).all()
        assert np.abs(rows[b, 0:3] - ref[0:3]).max() <= 1e-4 * scale, (b, rows[b], ref)
        assert abs(rows[b, 3] - ref[3]) <= 1e-4 * max(ref[3], 1.0)
        assert np.abs(rows[b, 4:7] - ref[4:7]).max() <= 1e-4 * scale * (1 + np.abs(hull).max()), (b, rows[b], ref)
    return rows


@pytest.mark.parametrize("sem", ["fftmesh", "renderer"])
def test_parity_on_waves(mw, sem):
    rng = np.random.default_rng(7)
    if sem == "fftmesh":
        p = workloads.fftmesh_params(256, choppiness=1.0)
        o = _ocean(mw, p)
        o.evaluate(2.3)
        vscale, span = 1.0 / o.params.t_division, 80.0
    else:
        o = _renderer(mw, 64)
        for dt in (0.3, 0.4):
            o.generate_texture(dt)
        vscale, span = 1.0, 20.0
    with o:
        for hull, tris in (H.icosphere(1.5), H.grid_hull(6, 10, 3.0, 5.0, 0.8)):
            ident = _bodies(mw, 6, rng, span, rotate=False)
            _parity(mw, o, hull, tris, ident, 0.0, 0.0, vscale, identity=True)
            _parity(mw, o, hull, tris, ident, 40.0, 90.0, vscale, identity=True)
            rot = _bodies(mw, 6, rng, span)
            _parity(mw, o, hull, tris, rot, 0.0, 0.0, vscale)
            _parity(mw, o, hull, tris, rot, 25.0, 0.0, vscale)
            _parity(mw, o, hull, tris, rot, 0.0, 60.0, vscale)


def test_reproducible_bit_for_bit(mw):
    """repeated calls, host vs device form, body k alone vs inside a batch of 1000, and (drag off) any velocity_scale: the same bits"""
    import torch
    p = workloads.fftmesh_params(1024, choppiness=1.2)
    rng = np.random.default_rng(3)
    hull, tris = H.icosphere(2.0)
    bodies = _bodies(mw, 1000, rng, 450.0, dy=(-2.0, 2.0))
    with _ocean(mw, p) as o:
        o.evaluate(4.0)
        for lin, quad in ((0.0, 0.0), (30.0, 70.0)):
            a = o.hull_forces(hull, tris, bodies, linear_drag=lin, quadratic_drag=quad)
            assert np.isfinite(a).all() and (a[:, 3] > 0).any()
            assert np.array_equal(_bits(o.hull_forces(hull, tris, bodies, linear_drag=lin, quadratic_drag=quad)), _bits(a))
            for k in (0, 1, 517, 999):
                one = o.hull_forces(hull, tris, bodies[k:k + 1], linear_drag=lin, quadratic_drag=quad)
                assert np.array_equal(_bits(one[0]), _bits(a[k])), k
            d_h = torch.from_numpy(hull).cuda()
            d_t = torch.from_numpy(tris).cuda()
            d_b = torch.from_numpy(bodies).cuda()
            d_o = torch.empty((1000, 8), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            o.hull_forces_device(d_h.data_ptr(), len(hull), d_t.data_ptr(), len(tris), d_b.data_ptr(), 1000, d_o.data_ptr(),
                                 linear_drag=lin, quadratic_drag=quad)
            o.synchronize()
            assert np.array_equal(_bits(d_o.cpu().numpy()), _bits(a))
        a = o.hull_forces(hull, tris, bodies)
        assert np.array_equal(_bits(o.hull_forces(hull, tris, bodies, velocity_scale=123.0)), _bits(a))
        b = o.hull_forces(hull, tris, bodies, linear_drag=30.0, velocity_scale=2.0)
        assert not np.array_equal(_bits(b), _bits(o.hull_forces(hull, tris, bodies, linear_drag=30.0, velocity_scale=3.0)))


def test_hull_forces_change_no_state(mw):
    """frames, timer, phase and query answers are bit-identical with and without hull calls in between"""
    hull, tris = H.icosphere(1.5)
    rng = np.random.default_rng(1)
    bodies = _bodies(mw, 8, rng, 60.0)
    p = workloads.fftmesh_params(256)
    xz = S.rest_plane(256, 1.0)[::97] * 0.9

    def fft_run(with_hull):
        out = []
        with _ocean(mw, p) as o:
            for k in range(3):
                v, n, c = o.update(0.03)
                if with_hull:
                    o.hull_forces(hull, tris, bodies); o.hull_forces(hull, tris, bodies, linear_drag=5.0, quadratic_drag=5.0)
                out += [v, n, c, np.float32(o.timer), o.query_surface(xz, mode="world"), o.query_velocity(xz, mode="world")]
            out += [o.evaluate(2.5)[0]]
        return out

    a, b = fft_run(False), fft_run(True)
    assert all(np.array_equal(_bits(np.atleast_1d(x)), _bits(np.atleast_1d(y))) for x, y in zip(a, b))
    rb = _bodies(mw, 4, rng, 5.0)

    def or_run(with_hull):
        out = []
        with _renderer(mw, 16) as r:
            for k in range(2):
                t = r.generate_texture(0.02)
                if with_hull:
                    r.hull_forces(hull, tris, rb); r.hull_forces(hull, tris, rb, linear_drag=5.0)
                out += list(t) + [r.get_phase(), r.query_surface(xz[:10] * 0.05, mode="world")]
            fr = r.generate_texture_steps([0.01, 0.02, 0.03])
            if with_hull:
                r.hull_forces(hull, tris, rb, frame=1); r.hull_forces(hull, tris, rb, frame=2, linear_drag=5.0)
            out += list(fr) + [r.get_phase(), r.query_surface(xz[:10] * 0.05, mode="world", frame=1), r.displace_mesh()[0]]
        return out

    a, b = or_run(False), or_run(True)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_frame_and_state_rules(mw, oracle):
    hull, tris = H.box(1.0, 1.0, 1.0)
    body = mw.pack_bodies([[0.3, 0.0, -0.2]])
    p = workloads.fftmesh_params(64)
    with _ocean(mw, p) as o:
        with pytest.raises(mw.MistralWaterError) as e:
            o.hull_forces(hull, tris, body)
        assert e.value.status == mw.MW_ESTATE  # no frame yet
        o.evaluate(1.0)
        o.hull_forces(hull, tris, body, linear_drag=1.0)
        h0, h0c = oracle.generate_spectrum(p, 3)
        o.set_spectrum(h0, h0c)
        o.hull_forces(hull, tris, body)  # drag off: the surface query's rules, the latest frame stays readable
        with pytest.raises(mw.MistralWaterError) as e:
            o.hull_forces(hull, tris, body, quadratic_drag=1.0)
        assert e.value.status == mw.MW_ESTATE and b"different instants" in mw.lib().mw_last_error()
        o.evaluate(1.0)
        o.hull_forces(hull, tris, body, quadratic_drag=1.0)
        with pytest.raises(mw.MistralWaterError) as e:
            o.hull_forces(hull, tris, body, frame=0)
        assert e.value.status == mw.MW_EINVAL
    with _renderer(mw, 32) as r:
        fr = r.generate_texture_steps([0.05, 0.1, 0.07])
        rb = mw.pack_bodies([[1.0, 0.0, 2.0], [-3.0, 0.2, 1.0]])
        for k in range(3):  # drag off: frame k of the steps call reads that frame's surface
            rows = r.hull_forces(hull, tris, rb, frame=k)
            x = H.transform(rb, hull).astype(np.float32)
            d, u, res = _water_at(r, x, frame=k)
            assert np.array_equal(_bits(rows[:, 7]), _bits(res.max(1)))
        assert not np.array_equal(r.hull_forces(hull, tris, rb, frame=0), r.hull_forces(hull, tris, rb, frame=2))
        r.hull_forces(hull, tris, rb, frame=2, linear_drag=3.0)  # drag on: the last frame of the steps call only
        with pytest.raises(mw.MistralWaterError) as e:
            r.hull_forces(hull, tris, rb, frame=1, linear_drag=3.0)
        assert e.value.status == mw.MW_EINVAL
        with pytest.raises(mw.MistralWaterError) as e:
            r.hull_forces(hull, tris, rb, frame=3)
        assert e.value.status == mw.MW_EINVAL
        r.advance_phase([0.01])
        r.hull_forces(hull, tris, rb)
        with pytest.raises(mw.MistralWaterError) as e:
            r.hull_forces(hull, tris, rb, linear_drag=3.0)
        assert e.value.status == mw.MW_ESTATE
        del fr
    with mw.Ocean(resolution=8, length=27.155, wind=(14.45, 12.0), amplitude=0.41, choppiness=1.5, semantics=mw.MW_SEM_OCEANRENDERER,
                  device=0, ntiles=2) as b:
        b.generate_texture(0.01)
        with pytest.raises(mw.MistralWaterError) as e:
            b.hull_forces(hull, tris, body)
        assert e.value.status == mw.MW_EINVAL


def test_error_statuses(mw):
    import ctypes as C
    L = mw.lib()
    _p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    hull, tris = H.box(1.0, 1.0, 1.0)
    body = mw.pack_bodies([[0.0, 0.0, 0.0]])
    out = np.zeros((1, 8), np.float32)
    good = np.array([RHO, G, 0, 0, 1], np.float32)
    with _ocean(mw, workloads.fftmesh_params(64)) as o:
        o.evaluate(1.0)
        h = o._h

        def call(hh=_p(hull), nv=8, tt=_p(tris), nt=12, bb=_p(body), nb=1, cf=_p(good), it=0, oo=_p(out), frame=-1):
            return L.mw_ocean_hull_forces(h, frame, hh, nv, tt, nt, bb, nb, cf, it, oo)
        assert call() == mw.MW_OK and np.isfinite(out).all()
        for kw in (dict(hh=None), dict(tt=None), dict(bb=None), dict(oo=None), dict(cf=None), dict(nv=2), dict(nt=0), dict(nb=-1),
                   dict(it=65), dict(it=-1), dict(frame=0), dict(nb=2 ** 30, nv=8)):
            assert call(**kw) == mw.MW_EINVAL, kw
        for bad in ([-1, G, 0, 0, 1], [RHO, np.nan, 0, 0, 1], [RHO, G, np.inf, 0, 1], [RHO, G, 0, -2, 1], [RHO, G, 0, 0, np.nan]):
            assert call(cf=_p(np.array(bad, np.float32))) == mw.MW_EINVAL, bad
        bt = tris.copy()
        bt[3, 2] = 8
        assert call(tt=_p(bt)) == mw.MW_EINVAL and b"index" in L.mw_last_error()
        out[:] = 5.0
        assert call(nb=0, hh=None, tt=None, bb=None, oo=None) == mw.MW_OK and (out == 5.0).all()


def test_out_of_range_device_indices_give_nan_rows(mw):
    """the device form reads no index it has not checked: a bad index makes every row NaN, and the call completes"""
    import torch
    hull, tris = H.icosphere(1.0)
    rng = np.random.default_rng(2)
    bodies = _bodies(mw, 3, rng, 20.0)
    with _ocean(mw, workloads.fftmesh_params(64)) as o:
        o.evaluate(1.0)
        for bad in (len(hull), -1, 2 ** 31 - 1):
            t = tris.copy()
            t[100, 1] = bad
            d_h, d_t, d_b = torch.from_numpy(hull).cuda(), torch.from_numpy(t).cuda(), torch.from_numpy(bodies).cuda()
            d_o = torch.zeros((3, 8), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            o.hull_forces_device(d_h.data_ptr(), len(hull), d_t.data_ptr(), len(t), d_b.data_ptr(), 3, d_o.data_ptr(), linear_drag=1.0)
            o.synchronize()
            assert torch.isnan(d_o).all()
        good = o.hull_forces(hull, tris, bodies)
        assert np.isfinite(good).all()
