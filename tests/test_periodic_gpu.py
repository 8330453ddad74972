"""GPU tier of the periodic surface (mw_ocean_set_periodic, include/mistral_water.h) through the C ABI.

The tiled kernels are compiled without floating-point contraction (csrc/surface_tiled.hip), so the reference is the g++ build of the same
MW_HD functions (tests/periodic_shim.cpp) run on the library's own vertex arrays: queries, hull rows and both plans of the bodies must
equal it bit for bit.  Shapes: the smallest grid of each transform family and both frame layouts -- FFTMesh 64^2 (unit_width 1, choppiness
1.5: folds), 256^2 (unit_width 0.5, length 128) and the chirp-z grid N = 100, L = 100."""
import ctypes as C

import numpy as np
import pytest

import hull_ref as H
import periodic_ref as PR
import surface_ref as S
import workloads

pytestmark = pytest.mark.gpu
bits = PR.bits
RHO, G = 1000.0, 9.81

GRIDS = {"fft64": dict(N=64, uw=1.0, chop=1.5), "fft256": dict(N=256, uw=0.5, chop=0.46), "czt100": dict(N=100, uw=1.0, chop=0.46)}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return PR.build_shim(str(tmp_path_factory.mktemp("psg") / "libperiodic_shim.so"))


def _ocean(mw, name, t=1.7):
    """the handle of a grid with one frame made, and that frame's arrays: vertices, normals, colours (RGBA), velocity"""
    g = GRIDS[name]
    L = g["N"] * g["uw"]
    p = workloads.fftmesh_params(int(L), choppiness=g["chop"])   # the amplitude that keeps the waves O(1) on a patch of this length
    o = mw.Ocean(resolution=g["N"], unit_width=g["uw"], length=L, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                 choppiness=g["chop"], gravity=p.gravity, seed=3, device=0)
    v, n, c = o.evaluate(t)
    return o, dict(R=g["N"], uw=g["uw"], P=PR.period(g["N"], g["uw"]), vert=v, norm=n, col=c, vel=o.velocity())


def _device(fn, xz, width, **kw):
    import torch
    d_xz = torch.from_numpy(np.ascontiguousarray(xz, np.float32)).cuda()
    d_out = torch.zeros((len(xz), width), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    fn(d_xz.data_ptr(), len(xz), d_out.data_ptr(), **kw)
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


# ---- queries --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(GRIDS))
def test_device_equals_the_shim_bit_for_bit(mw, shim, name):
    o, m = _ocean(mw, name)
    rng = np.random.default_rng(len(name))
    far = m["P"] * 2.0 ** 20
    xz = np.concatenate([PR.tile_points(m["R"], m["uw"], 11500, rng, tiles=3),
                         np.array([[np.nan, 0], [0, np.inf], [far + 2 * m["P"], 0], [0, -far + 2 * m["P"]], [3e38, -3e38]], np.float32)])
    assert len(xz) >= 20000
    with o:
        o.set_periodic(True)
        assert o.periodic and o.period == m["P"]
        for mode, code in (("rest", 0), ("world", 1)):
            want = PR.query_raw(shim, m["R"], m["uw"], m["P"], m["vert"], m["norm"], m["col"], 4, code, xz)
            host = o.query_surface(xz, mode=mode)
            assert np.array_equal(bits(host), bits(want)), (mode, int((bits(host) != bits(want)).any(1).sum()))
            o.synchronize()
            assert np.array_equal(bits(_device(o.query_surface_device, xz, 8, mode=mode)), bits(want))
            vwant = PR.velocity(shim, m["R"], m["uw"], m["P"], m["vert"], m["vel"], code, xz)
            vhost = o.query_velocity(xz, mode=mode)
            assert np.array_equal(bits(vhost), bits(vwant)), mode
            assert np.array_equal(bits(_device(o.query_velocity_device, xz, 4, mode=mode)), bits(vwant))
            assert np.isfinite(host[:-5]).all() and np.isnan(host[[-5, -4, -3, -1]]).all() and np.isnan(vhost[[-5, -4, -3, -1]]).all()
            assert np.isfinite(host[-2]).all()                      # 2^20 - 2 tiles out is still answered
            if mode == "world" and name != "fft64":                 # below the fold limit every point is found, in whatever tile
                assert host[:-5, 7].max() <= 1e-4


def test_translation_by_whole_tiles_is_exact_on_the_device(mw):
    o, m = _ocean(mw, "fft64")
    q = PR.base_points(m["R"], m["uw"], 400, np.random.default_rng(2), step=2.0 ** -8)
    P = m["P"]
    with o:
        o.set_periodic(True)
        for mode in ("rest", "world"):
            base, vbase = o.query_surface(q, mode=mode), o.query_velocity(q, mode=mode)
            assert np.isfinite(base).all()
            for kx in range(-3, 4):
                for kz in range(-3, 4):
                    sh = np.array([kx * P, kz * P], np.float32)
                    out = o.query_surface(q + sh, mode=mode)
                    want = base.copy()
                    want[:, 0] = base[:, 0] + sh[0]
                    want[:, 2] = base[:, 2] + sh[1]
                    assert np.array_equal(bits(out), bits(want)), (mode, kx, kz)
                    assert np.array_equal(bits(o.query_velocity(q + sh, mode=mode)), bits(vbase)), (mode, kx, kz)


# ---- hull forces ----------------------------------------------------------------------------------------------------------
def _boxes(mw, m, rng):
    """64 boxes afloat: 16 on the base footprint, the same 16 shifted by whole tiles, 16 straddling the x seam and 16 the z seam (the far
    corners 1.75 past the last grid line: off, the walk clamps there, more than a cell away)"""
    rc = S.rest_coords(m["R"], m["uw"])
    x0, hi, P = float(rc[0]), float(rc[-1]), m["P"]
    mid = hi + m["uw"] / 2
    base = rng.uniform(x0 + 6, hi - 6, (16, 2))
    shifted = base + rng.integers(1, 4, (16, 2)) * rng.choice([-1, 1], (16, 2)) * P
    along = rng.uniform(x0 + 6, hi - 6, 16)
    xz = np.concatenate([base, shifted, np.stack([np.full(16, mid), along], 1), np.stack([along, np.full(16, mid)], 1)])
    return xz, H.box(3.0, 1.0, 3.0)


@pytest.mark.parametrize("drag", [False, True], ids=["buoyancy", "drag"])
def test_hull_forces_on_shifted_and_straddling_hulls(mw, shim, drag):
    o, m = _ocean(mw, "fft256")
    rng = np.random.default_rng(5)
    xz, (hull, tris) = _boxes(mw, m, rng)
    kw = dict(linear_drag=30.0, quadratic_drag=60.0) if drag else {}
    with o:
        o.set_periodic(True)
        eta = o.query_surface(xz, mode="world")[:, 1]
        bodies = mw.pack_bodies(np.stack([xz[:, 0], eta, xz[:, 1]], 1), velocity=rng.standard_normal((64, 3)),
                                angular_velocity=0.2 * rng.standard_normal((64, 3)))
        o.set_periodic(False)
        off = o.hull_forces(hull, tris, bodies, **kw)
        lost = np.isnan(off).any(1) | (off[:, 7] > m["uw"])
        assert not lost[:16].any() and lost[16:].all(), (off[:, 7],)          # what fails without the feature
        o.set_periodic(True)
        rows = o.hull_forces(hull, tris, bodies, **kw)
        assert np.isfinite(rows).all() and (rows[:, 7] <= 1e-4).all() and (rows[:, 3] > 0).all()
        cf = np.array([RHO, G, kw.get("linear_drag", 0.0), kw.get("quadratic_drag", 0.0), 1.0 / o.params.t_division], np.float32)
        _, want = PR.hull_forces(shim, m["R"], m["uw"], m["P"], m["vert"], m["vel"], hull, tris, bodies, cf)
        assert np.array_equal(bits(rows), bits(want))
        for b in range(64):                                                     # a body alone: the bits it has in the batch
            assert np.array_equal(bits(o.hull_forces(hull, tris, bodies[b:b + 1], **kw)[0]), bits(rows[b])), b
        # the device form
        import torch
        d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (hull, tris, bodies)]
        d_o = torch.zeros((64, 8), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        o.hull_forces_device(d[0].data_ptr(), len(hull), d[1].data_ptr(), len(tris), d[2].data_ptr(), 64, d_o.data_ptr(), **kw)
        o.synchronize()
        assert np.array_equal(bits(d_o.cpu().numpy()), bits(rows))


# ---- bodies ---------------------------------------------------------------------------------------------------------------
def _run_plan(mw, value, fn):
    old = mw.get_switch("MW_BODIES_PLAN")
    mw.set_switch("MW_BODIES_PLAN", value)
    try:
        return fn()
    finally:
        mw.set_switch("MW_BODIES_PLAN", old)


@pytest.mark.parametrize("drag", [False, True], ids=["buoyancy", "drag"])
def test_buoys_cross_the_seam_in_both_plans(mw, shim, drag):
    o, m = _ocean(mw, "fft256")
    rng = np.random.default_rng(9)
    rc = S.rest_coords(m["R"], m["uw"])
    x0, hi, P = float(rc[0]), float(rc[-1]), m["P"]
    hull0, tris = H.icosphere(0.6, 1)
    mass1, cen, I = mw.hull_mass_properties(hull0, tris, 500.0)
    hull = np.asarray(hull0 - cen, np.float32)
    n = 32
    # 16 toward the +x seam, 16 toward the -z one; 8 substeps of 0.125 s at 6 m/s carry them 6 m: through the seam, into the next tile
    along = rng.uniform(x0 + 8, hi - 8, n)
    px = np.where(np.arange(n) < 16, hi - 1.0, along)
    pz = np.where(np.arange(n) < 16, along, x0 + 1.0)
    vel = np.where((np.arange(n) < 16)[:, None], [6.0, 0.0, 0.4], [-0.3, 0.0, -6.0])
    kw = dict(linear_drag=10.0, quadratic_drag=20.0) if drag else {}
    with o:
        o.set_periodic(True)
        eta = o.query_surface(np.stack([px, pz], 1), mode="world")[:, 1]
        bodies = mw.pack_bodies(np.stack([px, eta, pz], 1), velocity=vel)
        mass = mw.pack_mass(np.full(n, mass1), I)
        run = lambda: o.step_bodies(hull, tris, bodies.copy(), mass, 1.0, substeps=8, return_forces=True, **kw)  # noqa: E731
        a, ra = _run_plan(mw, 0, run)
        b, rb = _run_plan(mw, 1, run)
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(ra), bits(rb))
        assert np.isfinite(a).all() and np.isfinite(ra).all() and (ra[:, 7] <= 1e-4).all()
        assert (a[:16, 0] > x0 + P).all() and (a[16:, 2] < x0).all()                     # every buoy is in the next tile
        cf = np.array([RHO, G, kw.get("linear_drag", 0.0), kw.get("quadratic_drag", 0.0), 1.0 / o.params.t_division], np.float32)
        for plan in (0, 1):
            sb, sr = PR.step_bodies(shim, m["R"], m["uw"], m["P"], m["vert"], m["vel"], hull, tris, bodies, mass, cf, 1.0, 8, plan)
            assert np.array_equal(bits(sb), bits(a)) and np.array_equal(bits(sr), bits(ra)), plan
        o.set_periodic(False)
        c, rc_ = _run_plan(mw, 1, run)
        assert (np.isnan(rc_).any(1) | (rc_[:, 7] > m["uw"])).all()                      # off: the same buoys are lost


# ---- the switch -----------------------------------------------------------------------------------------------------------
def test_on_then_off_leaves_the_bits_of_a_handle_that_never_had_it_on(mw):
    o, m = _ocean(mw, "fft64")
    rng = np.random.default_rng(4)
    xz = PR.tile_points(m["R"], m["uw"], 600, rng, tiles=1)
    hull0, tris = H.icosphere(0.8, 1)
    mass1, cen, I = mw.hull_mass_properties(hull0, tris, 500.0)
    hull = np.asarray(hull0 - cen, np.float32)
    p = np.stack([rng.uniform(-40, 40, 12), rng.uniform(-0.3, 0.3, 12), rng.uniform(-40, 40, 12)], 1)
    bodies, mass = mw.pack_bodies(p, velocity=rng.standard_normal((12, 3))), mw.pack_mass(np.full(12, mass1), I)

    def services():
        out = [o.query_surface(xz, mode="rest"), o.query_surface(xz, mode="world"), o.query_velocity(xz, mode="world"),
               o.hull_forces(hull, tris, bodies, linear_drag=5.0)]
        out += list(o.step_bodies(hull, tris, bodies.copy(), mass, 0.3, substeps=4, linear_drag=5.0, return_forces=True))
        return out
    with o:
        before = services()
        frame = o.evaluate(1.7)
        assert np.isnan(before[0]).any()                                                 # rest points off the footprint: NaN, as ever
        o.set_periodic(True)
        on = services()
        assert np.isfinite(on[0]).all() and not np.array_equal(bits(on[1]), bits(before[1]))
        again = o.evaluate(1.7)                                                          # the switch changes no frame
        assert all(np.array_equal(bits(x), bits(y)) for x, y in zip(frame, again))
        o.set_periodic(False)
        assert not o.periodic
        after = services()
        for x, y in zip(before, after):
            assert np.array_equal(bits(x), bits(y))


def test_statuses_and_the_getter(mw):
    L = mw.lib()
    # the shipped scene: N = 12, length 12.39
    p = workloads.shipped_fftmesh_scene()
    with mw.Ocean(resolution=p.N, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                  choppiness=p.choppiness, device=0) as o:
        assert L.mw_ocean_set_periodic(o.handle, 1) == mw.MW_ENOTCOMMENSURATE and not o.periodic and o.period == 0.0
        assert L.mw_ocean_set_periodic(o.handle, 0) == mw.MW_OK
        assert L.mw_ocean_set_periodic(o.handle, 2) == mw.MW_EINVAL and L.mw_ocean_set_periodic(o.handle, -1) == mw.MW_EINVAL
    # an odd grid is anti-periodic
    with mw.Ocean(resolution=9, unit_width=1.0, length=9.0, device=0) as o:
        assert L.mw_ocean_set_periodic(o.handle, 1) == mw.MW_ENOTCOMMENSURATE and o.period == 0.0
    # OceanRenderer: the mesh does not tile; a batched handle has no single surface
    kw = dict(resolution=8, length=27.155, wind=(14.45, 12.0), amplitude=0.41, semantics=mw.MW_SEM_OCEANRENDERER, device=0)
    with mw.Ocean(**kw) as r:
        assert L.mw_ocean_set_periodic(r.handle, 1) == mw.MW_ESTATE and b"does not tile" in L.mw_last_error()
        assert L.mw_ocean_set_periodic(r.handle, 0) == mw.MW_OK and not r.periodic and r.period == 0.0
    with mw.Ocean(ntiles=2, **kw) as r:
        assert L.mw_ocean_set_periodic(r.handle, 1) == mw.MW_EINVAL
    # the chirp-z grid N = 100, L = 100: allowed; the getter; raycasts refuse; a new length that breaks the condition turns it off
    with mw.Ocean(resolution=100, unit_width=1.0, length=100.0, wind=(14.45, 12.0), amplitude=1e-6, device=0) as o:
        on, period = C.c_int32(-1), C.c_float(-1.0)
        assert L.mw_ocean_get_periodic(o.handle, C.byref(on), C.byref(period)) == mw.MW_OK and on.value == 0 and period.value == 100.0
        assert L.mw_ocean_get_periodic(o.handle, None, C.byref(period)) == mw.MW_OK and L.mw_ocean_get_periodic(o.handle, C.byref(on), None) == mw.MW_OK
        o.evaluate(0.5)
        hit_before = o.raycast([[0.0, 10.0, 0.0]], [[0.0, -1.0, 0.0]])[1]
        assert hit_before[0, 0] >= 0
        o.set_periodic(True)
        assert o.periodic and o.period == 100.0
        rays = mw.Ocean.pack_rays([[0.0, 10.0, 0.0]], [[0.0, -1.0, 0.0]])
        out, hit = np.full((1, 8), 7.0, np.float32), np.full((1, 2), 7, np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
        assert L.mw_ocean_raycast(o.handle, -1, vp(rays), 1, vp(out), vp(hit)) == mw.MW_ESTATE and b"do not tile" in L.mw_last_error()
        assert L.mw_ocean_raycast_device(o.handle, -1, None, 0, None, None) == mw.MW_ESTATE
        assert (out == 7.0).all() and (hit == 7).all()
        o.reinit_spectrum(length=63.0)
        assert not o.periodic and o.period == 0.0
        assert L.mw_ocean_set_periodic(o.handle, 1) == mw.MW_ENOTCOMMENSURATE
        o.reinit_spectrum(length=100.0)
        assert not o.periodic and o.period == 100.0                                      # it stays off until asked for again
        o.evaluate(0.5)
        assert o.raycast([[0.0, 10.0, 0.0]], [[0.0, -1.0, 0.0]])[1][0, 0] == hit_before[0, 0]
