"""GPU tier of draught (mw_ocean_set_draught, include/mistral_water.h) through the C ABI.

* with draught on every kernel of the hull family is one compiled without floating-point contraction (the vertex kernel of
  csrc/water_column.hip, then the strict rows and integration of csrc/surface_tiled.hip), so the reference of every row and every stepped
  state is the g++ build of the same MW_HD functions with the summation order restated by hand (tests/draught_shim.cpp, hull_order.h) run on
  the device's own layer arrays: bit for bit, on the one footprint and on the tiling, host and device forms, drag off and on;
* the Smith effect through the whole stack: a one-bin spectrum, 16 spars a sixteenth of a wavelength apart;
* the state rules, and that the switch moves nothing else and leaves nothing behind when it is switched off again."""
import ctypes as C

import numpy as np
import pytest

import draught_ref as DR
import hull_ref as H
import periodic_ref as PR
import test_hull_sizes_gpu as THS
import workloads

pytestmark = pytest.mark.gpu
f32 = np.float32
bits = DR.bits
VSCALE = 0.5
DRAG = dict(linear_drag=30.0, quadratic_drag=60.0)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return DR.build_shim(str(tmp_path_factory.mktemp("draughtg") / "libdraught_shim.so"))


def _ocean(mw, p, seed=3):
    return mw.Ocean(resolution=p.N, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                    choppiness=p.choppiness, gravity=p.gravity, seed=seed, device=0)


def _depths(L):
    return np.concatenate([[0.0], 0.25 * 1.45 ** np.arange(L - 1)]).astype(f32)   # geometric; L = 16 reaches 45


def _layers(o, L):
    arr = [o.column_layer_arrays(l) for l in range(L)]
    return np.stack([a[0] for a in arr]), np.stack([a[1] for a in arr])


def _status(mw, fn, *a, **kw):
    with pytest.raises(mw.MistralWaterError) as e:
        fn(*a, **kw)
    return e.value.status


def _coeffs(drag):
    return DR.coeffs(velocity_scale=VSCALE, **(DRAG if drag else {}))


def _kw(drag):
    return dict(velocity_scale=VSCALE, **(DRAG if drag else {}))


def _forces_device(o, hull, tris, bodies, drag):
    import torch
    d_hull, d_tris = torch.from_numpy(np.ascontiguousarray(hull, f32)).cuda(), torch.from_numpy(np.ascontiguousarray(tris, np.int32)).cuda()
    d_b = torch.from_numpy(np.ascontiguousarray(bodies, f32)).cuda()
    d_out = torch.zeros((len(bodies), 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    o.hull_forces_device(d_hull.data_ptr(), len(hull), d_tris.data_ptr(), len(tris), d_b.data_ptr(), len(bodies), d_out.data_ptr(), **_kw(drag))
    o.synchronize()
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


def _step_device(o, hull, tris, bodies, mass, dt, substeps, drag):
    import torch
    d_hull, d_tris = torch.from_numpy(np.ascontiguousarray(hull, f32)).cuda(), torch.from_numpy(np.ascontiguousarray(tris, np.int32)).cuda()
    d_b, d_m = torch.from_numpy(np.ascontiguousarray(bodies, f32)).cuda(), torch.from_numpy(np.ascontiguousarray(mass, f32)).cuda()
    d_out = torch.zeros((len(bodies), 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    o.step_bodies_device(d_hull.data_ptr(), len(hull), d_tris.data_ptr(), len(tris), d_b.data_ptr(), d_m.data_ptr(), len(bodies), dt,
                         substeps=substeps, d_out=d_out.data_ptr(), **_kw(drag))
    o.synchronize()
    torch.cuda.synchronize()
    return d_b.cpu().numpy(), d_out.cpu().numpy()


def _poses(o, n, rng, periodic, half, dmax, reach):
    """n bodies, n >= 4: afloat ones near the surface (upright within 15 degrees, moving and turning) -- over -3..3 tiles on a periodic
    handle, the first across the seam between two tiles; inside the footprint less the hull's reach otherwise -- and in the last three
    slots a NaN pose, a hull in the air and a hull below the deepest layer"""
    assert n >= 4
    if periodic:
        pts = PR.tile_points(o.N, 1.0, 4 * n, rng, tiles=3)       # uniform, seam strips and tile corners over 7 x 7 tiles
        xz = pts[rng.permutation(len(pts))[:n]].astype(np.float64)
        xz[0] = [half + 0.7, -3.3]          # the seam: the base tile ends at rest coordinate half + 1/2
    else:
        xz = rng.uniform(-half + reach, half - reach, (n, 2))
    eta = o.query_surface(xz.astype(f32))[:, 1]
    p = np.stack([xz[:, 0], eta + rng.uniform(-0.4, 0.2, n), xz[:, 1]], 1)
    p[-2, 1] = 3.0 * reach + 5.0                  # in the air
    p[-1, 1] = -float(dmax) - 3.0 * reach - 2.0   # below the deepest layer
    b = DR.pack(p, H.upright_quaternions(n, rng), rng.standard_normal((n, 3)) * 0.8, rng.standard_normal((n, 3)) * 0.3)
    b[-3, 0] = np.nan
    return b


def _batches(o, nb, rng, periodic, half, dmax, reach):
    """calls of exactly nb bodies whose union holds the three special poses: one call for nb >= 4, four calls of one body, two of two"""
    pool = _poses(o, max(nb, 4), rng, periodic, half, dmax, reach)
    return [pool[k:k + nb] for k in range(0, len(pool), nb)]


HULLS = [("spar", 1), ("spar", 32), ("spar", 33), ("icosphere", 2), ("edge255", 5), ("edge256", 5), ("edge257", 5)]


def _hull(name):
    if name == "spar":
        return DR.spar(), 8.5
    if name == "icosphere":
        return H.icosphere(1.5, 2), 1.5
    return H.edge_hull(int(name[4:])), 4.5


# ---- 1. device == shim, bit for bit, on the device's own layers ----------------------------------------------------------------------
@pytest.mark.parametrize("periodic", [False, True], ids=["footprint", "periodic"])
@pytest.mark.parametrize("L", [2, 16])
def test_device_equals_the_shim_bit_for_bit(mw, shim, L, periodic):
    """nbodies * nverts = 8, 256 and 264 with the spar (8 vertices: one lane group, exactly one workgroup, one more than a workgroup),
    324 with the icosphere; 255, 256 and 257 triangles with the edge hulls (the chunk edge).  Every batch of four or more bodies ends with
    a NaN pose, a hull in the air and a hull below the deepest layer; the batches of one and two bodies are called four and two times so
    that they see them too."""
    p = workloads.fftmesh_params(64, choppiness=1.0)
    depths = _depths(L)
    rng = np.random.default_rng(100 * L + periodic)
    with _ocean(mw, p) as o:
        o.set_column(depths)
        o.evaluate(1.7)
        if periodic:
            o.set_periodic(True)
        o.set_draught(True)
        assert o.draught
        pos, vel = _layers(o, L)
        P = o.period if periodic else 0.0
        seen = dict(nan=0, air=0, deep=0, wet=0)
        for name, nb in HULLS:
            (hull, tris), reach = _hull(name)
            if name == "spar":
                assert (len(hull), len(tris)) == (8, 12)
            if name == "icosphere":
                assert (len(hull), len(tris)) == (162, 320) and nb * len(hull) > 256
            for bodies in _batches(o, nb, rng, periodic, 32.0, depths[-1], reach):
                assert len(bodies) == nb
                for drag in (False, True):
                    slab, want = DR.forces(shim, 64, 1.0, P, depths, pos, vel, hull, tris, bodies, _coeffs(drag))
                    host = o.hull_forces(hull, tris, bodies, **_kw(drag))
                    dev = _forces_device(o, hull, tris, bodies, drag)
                    for got, form in ((host, "host"), (dev, "device")):
                        diff = (bits(got) != bits(want)).any(1)
                        assert not diff.any(), (name, nb, drag, form, int(diff.sum()), got[diff][:2], want[diff][:2])
                    nan = np.isnan(want).all(1)
                    air = ~nan & (want[:, :7] == 0).all(1)
                    deep = ~nan & (slab[:, :, 3] > depths[-1]).all(1)
                    assert (np.isnan(want).any(1) == nan).all() and np.isfinite(want[air, 7]).all()
                    seen["nan"] += int(nan.sum()); seen["air"] += int(air.sum()); seen["deep"] += int(deep.sum())
                    seen["wet"] += int((~nan & ~air & ~deep).sum())
                    if nb >= 4:
                        assert nan[-3] and air[-2] and deep[-1] and not nan[:-3].any() and (want[:-3, 3] > 0).all(), (name, nb)
                    if drag and (~nan & ~air).any():
                        assert (slab[~nan & ~air][:, :, 4:7] != 0).any()
        assert min(seen.values()) >= 2 * len(HULLS), seen


@pytest.mark.parametrize("periodic", [False, True], ids=["footprint", "periodic"])
def test_t16385_the_second_lap_of_the_reduce_equals_the_shim(mw, shim, periodic):
    """The hulls above stop at 257 triangles, 2 chunks.  t16385 (test_hull_sizes_gpu.hull_of) has 65: the smallest hull at which a lane of
    the reduce adds two partials (hull_body_sum's second lap), which draught reaches through the strict kernels it shares with the
    periodic handle.  Two bodies with the bottom sheet and so every sentinel wet (hull_ref.afloat_poses), on the periodic handle the
    second in another tile; L = 2, drag on, one forces call per handle."""
    p = workloads.fftmesh_params(64, choppiness=1.0)
    depths = _depths(2)
    hull, tris = THS.hull_of("t16385")
    rng = np.random.default_rng(65 + periodic)
    with _ocean(mw, p) as o:
        o.set_column(depths)
        o.evaluate(1.7)
        if periodic:
            o.set_periodic(True)
        o.set_draught(True)
        pos, vel = _layers(o, 2)
        P = o.period if periodic else 0.0
        eta = lambda xz: o.query_surface(np.ascontiguousarray(xz, f32))[:, 1].astype(np.float64)  # noqa: E731
        pq = H.afloat_poses(2, rng, 20.0, eta, tile_shift=(P, -2 * P) if periodic else None)
        bodies = DR.pack(*pq, rng.standard_normal((2, 3)) * 0.8, rng.standard_normal((2, 3)) * 0.3)
        slab, want = DR.forces(shim, 64, 1.0, P, depths, pos, vel, hull, tris, bodies, _coeffs(True))
        got = _forces_device(o, hull, tris, bodies, True)
    assert np.isfinite(want).all() and (slab[:, :, 4:7] != 0).any()
    assert len(H.sentinel_slots(len(tris))) == 5 and (want[:, 3] > 5 * 18.0 * 0.99).all()   # wet area: every sentinel, 18 each
    assert np.array_equal(bits(got), bits(want)), (got, want)


# ---- 2. stepping ----------------------------------------------------------------------------------------------------------------------
def _mass_rows(mw, hull, tris, n, density=600.0):
    m, _, I = mw.hull_mass_properties(hull, tris, density)
    return mw.pack_mass(np.full(n, m), np.broadcast_to(I, (n, 3, 3)))


@pytest.mark.parametrize("periodic", [False, True], ids=["footprint", "periodic"])
def test_stepping_equals_the_shim_bit_for_bit(mw, shim, periodic):
    p = workloads.fftmesh_params(64, choppiness=1.0)
    depths = _depths(5)
    rng = np.random.default_rng(40 + periodic)
    with _ocean(mw, p) as o:
        o.set_column(depths)
        o.evaluate(0.9)
        if periodic:
            o.set_periodic(True)
        o.set_draught(True)
        pos, vel = _layers(o, 5)
        P = o.period if periodic else 0.0
        for name, nb in (("spar", 33), ("icosphere", 6)):
            (hull, tris), reach = _hull(name)
            bodies = _poses(o, nb, rng, periodic, 32.0, depths[-1], reach)
            mass = _mass_rows(mw, hull, tris, nb)
            for drag in (False, True):
                wb, wr = DR.step(shim, 64, 1.0, P, depths, pos, vel, hull, tris, bodies, mass, _coeffs(drag), 0.08, 8)
                hb, hr = o.step_bodies(hull, tris, bodies.copy(), mass, 0.08, substeps=8, return_forces=True, **_kw(drag))
                db, dr = _step_device(o, hull, tris, bodies, mass, 0.08, 8, drag)
                for gb, gr, form in ((hb, hr, "host"), (db, dr, "device")):
                    assert np.array_equal(bits(gb), bits(wb)), (name, drag, form, "states")
                    assert np.array_equal(bits(gr), bits(wr)), (name, drag, form, "rows")
                assert np.isnan(wr[-3]).all() and np.array_equal(bits(wb[-3]), bits(bodies[-3]))         # the NaN pose stays as it was
                assert not np.array_equal(bits(wb[:-3, 0:3]), bits(bodies[:-3, 0:3])) and np.isfinite(wb[:-3]).all()
                # one substep: the returned row is hull_forces_device's
                _, r1 = _step_device(o, hull, tris, bodies, mass, 0.01, 1, drag)
                assert np.array_equal(bits(r1), bits(_forces_device(o, hull, tris, bodies, drag))), (name, drag)
            # an invalid mass row (device form: the host form refuses it): the body unchanged, a NaN row, the others as before
            bad = mass.copy()
            bad[1, 0] = -1.0
            bad[2, 1] = np.nan
            wb, wr = DR.step(shim, 64, 1.0, P, depths, pos, vel, hull, tris, bodies, bad, _coeffs(True), 0.08, 8)
            db, dr = _step_device(o, hull, tris, bodies, bad, 0.08, 8, True)
            assert np.array_equal(bits(db), bits(wb)) and np.array_equal(bits(dr), bits(wr))
            assert np.isnan(dr[1:3]).all() and np.array_equal(bits(db[1:3]), bits(bodies[1:3])) and np.isfinite(dr[0]).all()
            assert _status(mw, o.step_bodies, hull, tris, bodies.copy(), bad, 0.08, substeps=8) == mw.MW_EINVAL


# ---- 3. every grid path ------------------------------------------------------------------------------------------------------------
def test_the_shipped_scene_chirp_z_equals_the_shim(mw, shim):
    """N = 12, length 12.39: not commensurate, so the frame and every layer come from the chirp-z path and the handle cannot tile.
    Five spars scaled to that footprint (0.5 x 4 x 0.5, bottom at -2)."""
    p = workloads.shipped_fftmesh_scene()
    depths = np.array([0.0, p.length / 32, p.length / 8], f32)
    hull, tris = H.box(0.5, 4.0, 0.5)
    rng = np.random.default_rng(12)
    with _ocean(mw, p) as o:
        o.set_column(depths)
        o.evaluate(1.7)
        o.set_draught(True)
        assert _status(mw, o.set_periodic, True) == mw.MW_ENOTCOMMENSURATE
        pos, vel = _layers(o, 3)
        xz = rng.uniform(-4.0, 4.0, (5, 2))
        eta = o.query_surface(xz.astype(f32))[:, 1]
        bodies = DR.pack(np.stack([xz[:, 0], eta + rng.uniform(-0.2, 0.2, 5), xz[:, 1]], 1), H.upright_quaternions(5, rng),
                         rng.standard_normal((5, 3)) * 0.3, rng.standard_normal((5, 3)) * 0.2)
        for drag in (False, True):
            slab, want = DR.forces(shim, p.N, p.unit_width, 0.0, depths, pos, vel, hull, tris, bodies, _coeffs(drag))
            assert np.isfinite(want).all() and (want[:, 3] > 0).all() and (slab[:, :, 3] > depths[1]).any()
            assert np.array_equal(bits(o.hull_forces(hull, tris, bodies, **_kw(drag))), bits(want)), drag
            assert np.array_equal(bits(_forces_device(o, hull, tris, bodies, drag)), bits(want)), drag


# ---- 4. the Smith effect on the device ---------------------------------------------------------------------------------------------------
def test_smith_effect_on_the_device(mw):
    """One spectrum bin along x, wave number k = 2 pi 2 / 64 (kT = pi / 2 for the spar's draught T = 8), on the periodic 64^2 handle; 16
    spars in one call a sixteenth of the wavelength (2 units) apart.  The half range of F_y with draught on over the half range with
    draught off must be e^{-kT} to 2 %; the float64 composition on the device's own layers is first held to 1 %."""
    p = workloads.fftmesh_params(64, choppiness=1.0)
    j = 2
    k = 2 * np.pi * j / p.length
    depths = np.array([0.0, 4.0, 8.0, 16.0], f32)
    h0 = np.zeros((64, 64, 2), f32)
    h0[32 + j, 32] = (0.04, -0.03)
    hull, tris = DR.spar()
    want = np.exp(-k * DR.SPAR_DRAUGHT)
    half = lambda fy: (np.max(fy) - np.min(fy)) / 2
    with _ocean(mw, p) as o:
        o.set_spectrum(h0, np.zeros_like(h0))
        o.set_column(depths)
        v, _, _ = o.evaluate(0.6)
        o.set_periodic(True)
        eta = v[:, 1].reshape(64, 64)             # vertex (i, j) at i * 64 + j, x from i
        a = float(np.abs(eta).max())
        along_x = np.ptp(eta, axis=0).max() > np.ptp(eta, axis=1).max()
        assert 5e-3 < a < 0.5 and min(np.ptp(eta, axis=0).max(), np.ptp(eta, axis=1).max()) < 1e-3 * a   # one plane wave along one axis
        s, c = -14.9 + 2.0 * np.arange(16), np.full(16, 1.3)
        bodies = DR.pack(np.stack([s if along_x else c, np.zeros(16), c if along_x else s], 1))
        off = o.hull_forces(hull, tris, bodies, velocity_scale=VSCALE)
        o.set_draught(True)
        on = o.hull_forces(hull, tris, bodies, velocity_scale=VSCALE)
        pos, vel = _layers(o, 4)
        P = o.period
    col = DR.forces_f64(64, 1.0, P, depths, pos, vel, hull, tris, bodies, DR.coeffs())[0][:, 1]
    surf = DR.forces_f64(64, 1.0, P, depths, pos, vel, hull, tris, bodies, DR.coeffs(), depth="surface")[0][:, 1]
    r64, rdev = half(col) / half(surf), half(on[:, 1]) / half(off[:, 1])
    print("a %.4f  e^-kT %.5f  float64 on the device's layers %.5f (%.3f %%)  device %.5f (%.3f %%)" %
          (a, want, r64, 100 * (r64 / want - 1), rdev, 100 * (rdev / want - 1)))
    assert half(off[:, 1]) > 0.5 * DR.RHO * DR.G * 4.0 * a     # without draught the spar heaves as if it sat at the surface
    assert abs(r64 - want) <= 0.01 * want
    assert abs(rdev - want) <= 0.02 * want


# ---- 5. state rules -------------------------------------------------------------------------------------------------------------------
def _fleet_calls(mw, o, hull, tris, bodies, mass):
    import torch
    fx, ft, table = mw.pack_fleet([(hull, tris, len(bodies))])
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    dx, dt_, db, dm = d(fx), d(ft), d(bodies), d(mass)
    out = torch.zeros((len(bodies), 8), dtype=torch.float32, device="cuda")
    return [lambda: o.fleet_forces(fx, ft, table, bodies),
            lambda: o.step_fleet(fx, ft, table, bodies.copy(), mass, 0.01),
            lambda: o.fleet_forces_device(dx.data_ptr(), len(fx), dt_.data_ptr(), len(ft), table, db.data_ptr(), len(bodies), out.data_ptr()),
            lambda: o.step_fleet_device(dx.data_ptr(), len(fx), dt_.data_ptr(), len(ft), table, db.data_ptr(), dm.data_ptr(), len(bodies), 0.01)]


def _hull_calls(mw, o, hull, tris, bodies, mass, drag):
    return [lambda: o.hull_forces(hull, tris, bodies, **_kw(drag)),
            lambda: _forces_device(o, hull, tris, bodies, drag),
            lambda: o.step_bodies(hull, tris, bodies.copy(), mass, 0.01, **_kw(drag)),
            lambda: _step_device(o, hull, tris, bodies, mass, 0.01, 1, drag)]


def test_state_rules(mw):
    p = workloads.fftmesh_params(64)
    hull, tris = DR.spar()
    bodies = DR.pack([[1.0, 0.0, 2.0], [-7.0, 0.3, 11.0]])
    mass = _mass_rows(mw, hull, tris, 2)
    L = mw.lib()
    with _ocean(mw, p) as o:
        assert not o.draught
        for bad in (2, -1, 7):
            assert L.mw_ocean_set_draught(o.handle, bad) == mw.MW_EINVAL
        assert not o.draught
        o.set_draught(True)                       # no column has to be set yet
        assert o.draught
        on = C.c_int32(5)
        assert L.mw_ocean_get_draught(o.handle, C.byref(on)) == mw.MW_OK and on.value == 1
        assert L.mw_ocean_get_draught(o.handle, None) == mw.MW_OK
        for drag in (False, True):                # no column, no frame
            for call in _hull_calls(mw, o, hull, tris, bodies, mass, drag):
                assert _status(mw, call) == mw.MW_ESTATE
        o.evaluate(1.0)
        for drag in (False, True):                # a frame, no column
            for call in _hull_calls(mw, o, hull, tris, bodies, mass, drag):
                assert _status(mw, call) == mw.MW_ESTATE
            assert b"mw_ocean_set_column" in L.mw_last_error()
        # the calls' own argument checks come first
        assert _status(mw, o.hull_forces, hull[:2], tris, bodies) == mw.MW_EINVAL
        assert _status(mw, o.step_bodies, hull, tris, bodies.copy(), mass, 0.01, substeps=65) == mw.MW_EINVAL
        assert _status(mw, o.hull_forces, hull, tris, bodies, density=np.nan) == mw.MW_EINVAL
        o.set_column([0.0, 4.0, 8.0, 16.0])
        first = [call() for call in _hull_calls(mw, o, hull, tris, bodies, mass, True)]
        assert np.isfinite(first[0]).all() and np.array_equal(bits(first[0]), bits(first[1]))
        # the spectrum moved past the frame: MW_ESTATE with drag off too (without draught a drag-free call reads the surface alone)
        h0, h0c = o.get_spectrum()
        o.set_spectrum(h0, h0c)
        for drag in (False, True):
            for call in _hull_calls(mw, o, hull, tris, bodies, mass, drag):
                assert _status(mw, call) == mw.MW_ESTATE
        o.set_draught(False)
        assert np.isfinite(o.hull_forces(hull, tris, bodies)).all() and _status(mw, o.hull_forces, hull, tris, bodies, **_kw(True)) == mw.MW_ESTATE
        o.set_draught(True)
        o.evaluate(1.0)
        assert np.array_equal(bits(o.hull_forces(hull, tris, bodies, **_kw(True))), bits(first[0]))
        # the fleets refuse, and say why; with draught off they run
        for call in _fleet_calls(mw, o, hull, tris, bodies, mass):
            assert _status(mw, call) == mw.MW_ESTATE
            assert b"mw_ocean_set_draught" in L.mw_last_error()
        o.set_draught(False)
        for call in _fleet_calls(mw, o, hull, tris, bodies, mass):
            call()
        o.synchronize()
        o.set_draught(True)
        # releasing the column with draught on
        o.set_column(None)
        assert o.draught
        for drag in (False, True):
            for call in _hull_calls(mw, o, hull, tris, bodies, mass, drag):
                assert _status(mw, call) == mw.MW_ESTATE
        o.set_draught(False)
        assert np.isfinite(o.hull_forces(hull, tris, bodies, **_kw(True))).all()
        assert o.timer == 0.0 and not o.periodic
    # handles without a column refuse the switch with mw_ocean_set_column's status, on or off
    for kw in (dict(), dict(ntiles=2)):
        with mw.Ocean(resolution=8, length=27.155, wind=(14.45, 12.0), amplitude=0.41, choppiness=0.46, mult=1.5, semantics=mw.MW_SEM_OCEANRENDERER,
                      device=0, **kw) as r:
            assert _status(mw, r.set_draught, True) == mw.MW_EINVAL and _status(mw, r.set_draught, False) == mw.MW_EINVAL
            assert _status(mw, r.set_column, [0.0, 1.0]) == mw.MW_EINVAL
            assert not r.draught


# ---- 6. nothing else moves ----------------------------------------------------------------------------------------------------------
def _others(o, rng_seed=12):
    rng = np.random.default_rng(rng_seed)
    xz = rng.uniform(-28, 28, (500, 2)).astype(f32)
    q = np.stack([xz[:, 0], rng.uniform(-20, 1, 500), xz[:, 1]], 1).astype(f32)
    out = [o.query_surface(xz), o.query_velocity(xz), o.query_column(q), o.query_column(q, mode="rest")]
    if not o.periodic:
        rc, hit = o.raycast(np.stack([xz[:, 0], np.full(500, 20.0), xz[:, 1]], 1), np.tile([0.1, -1.0, 0.05], (500, 1)))
    else:
        rc, hit = o.raycast_tiled(np.stack([xz[:, 0], np.full(500, 20.0), xz[:, 1]], 1), np.tile([0.1, -1.0, 0.05], (500, 1)))
    return out + [rc, hit.astype(f32), o.velocity()]


@pytest.mark.parametrize("periodic", [False, True], ids=["footprint", "periodic"])
def test_the_switch_moves_nothing_else_and_leaves_nothing_behind(mw, periodic):
    p = workloads.fftmesh_params(64, choppiness=1.0)
    hull, tris = H.icosphere(1.5, 2)
    rng = np.random.default_rng(9)
    with _ocean(mw, p) as o:
        o.set_column(_depths(5))
        o.evaluate(1.7)
        if periodic:
            o.set_periodic(True)
        bodies = _poses(o, 12, rng, periodic, 32.0, 3.0, 1.5)
        mass = _mass_rows(mw, hull, tris, 12)
        hulls = lambda: [o.hull_forces(hull, tris, bodies, **_kw(True)),
                         *o.step_bodies(hull, tris, bodies.copy(), mass, 0.05, substeps=4, return_forces=True, **_kw(True))]
        before, hulls_before = _others(o), hulls()
        o.set_draught(True)
        during, hulls_during = _others(o), hulls()
        o.set_draught(False)
        after, hulls_after = _others(o), hulls()
    for k, (a, b, c) in enumerate(zip(before, during, after)):
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c)), k
    for k, (a, b, c) in enumerate(zip(hulls_before, hulls_during, hulls_after)):
        assert np.array_equal(bits(a), bits(c)), k                    # off again: the bits from before it was switched on
        assert not np.array_equal(bits(a), bits(b)), k                # on: the column's depths and velocities do change the rows
