"""GPU tier of the water column (mw_ocean_set_column / mw_ocean_query_column, include/mistral_water.h) through the C ABI.

* the layers the device builds against the float64 oracle's (tests/column_ref.py::layers_f64) on every grid path: FFT 64^2, FFT 256^2
  (the frame plan), the shipped non-commensurate N = 12 scene (chirp-z, one launch) and N = 100 (chirp-z, two launches);
* the column's kernels are compiled without floating-point contraction (csrc/water_column.hip), so the query's reference is the g++ build of
  the same MW_HD functions (tests/column_shim.cpp) run on the device's own layer arrays: bit for bit, both modes, both mesh types;
* the state rules, and that a column changes nothing any other service returns."""
import ctypes as C

import numpy as np
import pytest

import column_ref as CR
import hull_ref as H
import periodic_ref as PR
import surface_ref as S
import workloads

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return CR.build_shim(str(tmp_path_factory.mktemp("colg") / "libcol_shim.so"))


def _ocean(mw, p, seed=3):
    return mw.Ocean(resolution=p.N, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                    choppiness=p.choppiness, gravity=p.gravity, seed=seed, device=0)


def _params(oracle, name):
    if name == "shipped12":
        return workloads.shipped_fftmesh_scene()
    if name == "czt100":
        return oracle.Params(N=100, unit_width=1.0, length=100.0, wind_x=14.45, wind_y=12.0, amplitude=1.5e-8 * (1024.0 / 100) ** 2, choppiness=0.46)
    return workloads.fftmesh_params(int(name[3:]))


def _assert_field(got, ref, rel, tag, ulp_of=None):
    """workloads.assert_parity's vertex rule: rel * max|field| + 1 ulp of the stored value (a vertex stores rest + displacement)"""
    scale = max(float(np.abs(ref).max()), 1e-30)
    err = np.abs(got - ref)
    bound = rel * scale + np.abs(ref if ulp_of is None else ulp_of) * 2.0 ** -23
    assert (err <= bound).all(), f"{tag}: max excess {float((err - bound).max()):.3e}, max err / scale {float(err.max()) / scale:.3e}"


def _layers(o, L):
    """the device's layer arrays [L, N*N, 3] x 2, downloaded through mw_ocean_column_layers"""
    arr = [o.column_layer_arrays(l) for l in range(L)]
    return np.stack([a[0] for a in arr]), np.stack([a[1] for a in arr])


def _device(o, q, mode):
    import torch
    d_q = torch.from_numpy(np.ascontiguousarray(q, f32)).cuda()
    d_out = torch.zeros((len(q), 12), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    o.query_column_device(d_q.data_ptr(), len(q), d_out.data_ptr(), mode=mode)
    o.synchronize()
    torch.cuda.synchronize()
    return d_out.cpu().numpy()


# ---- the layers ----------------------------------------------------------------------------------------------------------------
# the frame's bound is the layer's bound (a layer is a frame of another spectrum): REL_TOL on the FFT path, 2e-5 on the direct paths
# (tests/test_gpu_parity.py, tests/test_velocity_gpu.py)
@pytest.mark.parametrize("name,rel", [("fft64", workloads.REL_TOL), ("fft256", workloads.REL_TOL), ("shipped12", 2e-5), ("czt100", 2e-5)])
def test_layers_match_the_oracle_and_layer_0_is_the_surface(mw, oracle, name, rel):
    p = _params(oracle, name)
    N, t = p.N, 1.7
    depths = np.array([0.0, p.length / 32, p.length / 8], f32)
    with _ocean(mw, p) as o:
        o.set_column(depths)
        assert np.array_equal(o.column, depths)
        v, _, _ = o.evaluate(t)
        h0, h0c = o.get_spectrum()
        pos, vel = _layers(o, 3)
        surface_vel = o.velocity()
    assert np.array_equal(bits(pos[0]), bits(v)) and np.array_equal(bits(vel[0]), bits(surface_vel))
    rpos, rvel = CR.layers_f64(p, h0.reshape(N, N, 2), h0c.reshape(N, N, 2), t, depths)
    rest = oracle.rest_mesh(p)[0].astype(np.float64)
    for l in (1, 2):
        _assert_field(pos[l] - rest, rpos[l] - rest, rel, f"{name} layer {l} positions", ulp_of=rpos[l])
        _assert_field(vel[l], rvel[l], rel, f"{name} layer {l} velocity")
        assert np.abs(rpos[l] - rest).max() < np.abs(rpos[l - 1] - rest).max()


# ---- device == shim, bit for bit, on the device's own layers ------------------------------------------------------------------------
def _depths(L):
    return np.concatenate([[0.0], 0.25 * 1.45 ** np.arange(L - 1)]).astype(f32)   # geometric; L = 16 reaches 45


def _points(N, periodic, rng, dmax):
    """20 000 world points and labels: over -3..3 tiles (seams and corners included) on a periodic handle, over and a little beyond the
    footprint otherwise; heights from the air down to below the deepest layer; a few rows without an answer"""
    if periodic:
        xz = PR.tile_points(N, 1.0, 11500, rng, tiles=3)[:19990]
    else:
        xz = rng.uniform(-N / 2 - 2, N / 2 + 2, (19990, 2)).astype(f32)
    y = rng.uniform(-1.3 * dmax, 1.5, len(xz))
    world = np.stack([xz[:, 0], y, xz[:, 1]], -1).astype(f32)
    rest = np.stack([xz[:, 0], rng.uniform(-0.02 * dmax, 1.02 * dmax, len(xz)), xz[:, 1]], -1).astype(f32)
    rest[:200, 1] = rng.choice([0.0, dmax], 200)
    bad = np.array([[np.nan, -1, 0], [0, np.nan, 0], [0, -1, np.inf], [0, np.inf, 0], [0, -np.inf, 0], [3e38, -1, -3e38], [0, 0.125, 0], [1, 0, 1],
                    [0, dmax, 0], [0.5, 0.25, 0.5]], f32)
    return np.concatenate([world, bad]), np.concatenate([rest, bad])


@pytest.mark.parametrize("periodic", [False, True], ids=["footprint", "periodic"])
@pytest.mark.parametrize("L", [2, 3, 16])
def test_device_equals_the_shim_bit_for_bit(mw, shim, L, periodic):
    p = workloads.fftmesh_params(64, choppiness=1.0)
    depths = _depths(L)
    rng = np.random.default_rng(10 * L + periodic)
    world, rest = _points(64, periodic, rng, float(depths[-1]))
    assert len(world) == 20000
    with _ocean(mw, p) as o:
        o.set_column(depths)
        o.evaluate(1.7)
        if periodic:
            o.set_periodic(True)
        pos, vel = _layers(o, L)
        P = o.period if periodic else 0.0
        for mode, code, q in (("world", CR.WORLD, world), ("rest", CR.REST, rest)):
            want = CR.query(shim, 64, 1.0, P, depths, pos, vel, code, q)
            host = o.query_column(CR.pad4(q), mode=mode)
            diff = (bits(host) != bits(want)).any(1)
            assert not diff.any(), (mode, int(diff.sum()), q[diff][:3], host[diff][:3], want[diff][:3])
            assert np.isnan(host[-10:-5]).all() and np.isfinite(host[-4:]).all()
            assert np.isfinite(host[:, CR.LAMBDA]).mean() > 0.7
            for n in (1, 255, 256, 257, 20000):
                part = o.query_column(CR.pad4(q[:n]), mode=mode)
                assert np.array_equal(bits(part), bits(want[:n])), (mode, n)
                dev = _device(o, CR.pad4(q[:n]), mode)
                assert np.array_equal(bits(dev), bits(want[:n])), (mode, n, "device form")
        if L == 16:   # every interval is populated and the scan went all the way down
            lam = host[:, CR.LAMBDA]
            assert (np.floor(lam[np.isfinite(lam)]) == 15).any()


def test_a_vertex_label_at_a_layer_depth_returns_the_layers_bits_on_the_device(mw):
    p = workloads.fftmesh_params(64)
    depths = _depths(4)
    rc = S.rest_coords(64, 1.0)
    X, Z = np.meshgrid(rc, rc, indexing="ij")
    with _ocean(mw, p) as o:
        o.set_column(depths)
        o.evaluate(0.5)
        pos, vel = _layers(o, 4)
        for l, d in enumerate(depths):
            out = o.query_column(np.stack([X.ravel(), np.full(X.size, d, f32), Z.ravel()], -1), mode="rest")
            want = pos[l].copy()
            want[:, 1] = want[:, 1] - d
            assert np.array_equal(bits(out[:, CR.PX:CR.PZ + 1]), bits(want)) and np.array_equal(bits(out[:, CR.UX:CR.UZ + 1]), bits(vel[l])), l
            assert (out[:, CR.LAMBDA] == l).all() and (out[:, CR.DEPTH] == d).all()


# ---- the periodic handle agrees with the surface services bit for bit ----------------------------------------------------------------
def test_on_a_periodic_handle_the_surface_fed_back_has_the_surface_services_bits(mw):
    p = workloads.fftmesh_params(64, choppiness=1.0)
    xz = PR.tile_points(64, 1.0, 4000, np.random.default_rng(8), tiles=3)
    with _ocean(mw, p) as o:
        o.set_column(_depths(4))
        o.evaluate(2.5)
        o.set_periodic(True)
        qs, qv = o.query_surface(xz, mode="world"), o.query_velocity(xz, mode="world")
        col = o.query_column(np.stack([xz[:, 0], qs[:, 1], xz[:, 1]], -1), mode="world")
    assert np.isfinite(col).all()
    assert np.array_equal(bits(col[:, CR.ETA]), bits(qs[:, 1])) and np.array_equal(bits(col[:, CR.RESIDUAL]), bits(qs[:, 7]))
    assert np.array_equal(bits(col[:, CR.UX:CR.UZ + 1]), bits(qv[:, :3])) and (col[:, CR.LAMBDA] == 0).all()
    assert np.array_equal(bits(col[:, CR.PX:CR.PZ + 1]), bits(qs[:, :3])) and (col[:, CR.DEPTH] == 0).all()


# ---- state ---------------------------------------------------------------------------------------------------------------------
def _status(mw, fn, *a):
    with pytest.raises(mw.MistralWaterError) as e:
        fn(*a)
    return e.value.status


def test_state_rules(mw):
    p = workloads.fftmesh_params(64)
    q = np.array([[0.5, -1.0, 0.25], [3.0, -4.0, -7.0]], f32)
    depths = _depths(3)
    with _ocean(mw, p) as o:
        assert len(o.column) == 0
        assert _status(mw, o.query_column, q) == mw.MW_ESTATE            # before set_column (and before a frame)
        o.evaluate(1.0)
        assert _status(mw, o.query_column, q) == mw.MW_ESTATE            # a frame, no column
        assert _status(mw, o.column_layers, 0) == mw.MW_ESTATE
    with _ocean(mw, p) as o:
        o.set_column(depths)
        assert _status(mw, o.query_column, q) == mw.MW_ESTATE            # a column, no frame
        o.evaluate(1.0)
        a = o.query_column(q)
        assert np.isfinite(a).all() and np.array_equal(bits(o.query_column(q)), bits(a))   # a second identical call: identical bits
        h0, h0c = o.get_spectrum()
        o.set_spectrum(h0, h0c)
        assert _status(mw, o.query_column, q) == mw.MW_ESTATE            # the spectrum moved past the frame
        assert _status(mw, o.column_layers, 1) == mw.MW_ESTATE
        o.evaluate(1.0)
        assert np.array_equal(bits(o.query_column(q)), bits(a))          # the same spectrum again: the rebuilt layers are the same
        # argument rules
        for bad in ([0.0], [0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.5, 1.0], [0.0, np.inf], [0.0, np.nan], np.arange(17.0)):
            assert _status(mw, o.set_column, bad) == mw.MW_EINVAL, bad
        assert np.array_equal(o.column, depths)                          # a refused call leaves the column alone
        assert np.array_equal(bits(o.query_column(q)), bits(a))
        out = np.full((2, 12), 7.0, f32)
        L, xyz = mw.lib(), CR.pad4(q)
        ptr = lambda x: x.ctypes.data_as(C.c_void_p)
        assert L.mw_ocean_query_column(o.handle, 0, 1, ptr(xyz), 2, 0, ptr(out)) == mw.MW_EINVAL       # frame != -1
        assert L.mw_ocean_query_column(o.handle, -1, 2, ptr(xyz), 2, 0, ptr(out)) == mw.MW_EINVAL      # a bad mode
        assert L.mw_ocean_query_column(o.handle, -1, 1, ptr(xyz), 2, 65, ptr(out)) == mw.MW_EINVAL     # iterations
        assert L.mw_ocean_query_column(o.handle, -1, 1, None, 2, 0, ptr(out)) == mw.MW_EINVAL          # a NULL array
        assert L.mw_ocean_query_column(o.handle, -1, 1, ptr(xyz), -1, 0, ptr(out)) == mw.MW_EINVAL
        assert L.mw_ocean_query_column(o.handle, -1, 1, ptr(xyz), 2 ** 32 - 255, 0, ptr(out)) == mw.MW_EINVAL
        assert L.mw_ocean_query_column(o.handle, -1, 1, None, 0, 0, None) == mw.MW_OK                  # n == 0 does nothing
        assert (out == 7).all()
        assert _status(mw, o.column_layers, 3) == mw.MW_EINVAL and _status(mw, o.column_layers, -1) == mw.MW_EINVAL
        import torch
        d = torch.zeros(64, dtype=torch.float32, device="cuda")
        assert _status(mw, o.query_column_device, d.data_ptr() + 4, 1, d.data_ptr() + 64) == mw.MW_EINVAL   # misaligned
        assert _status(mw, o.query_column_device, d.data_ptr(), 1, d.data_ptr() + 72) == mw.MW_EINVAL
        # no column call moved the timer, the frame or the switch
        assert o.timer == 0.0 and not o.periodic
        # other depths take effect; releasing the column is MW_ESTATE again
        o.set_column([0.0, 0.5, 30.0])
        b = o.query_column(q)
        assert np.isfinite(b).all() and not np.array_equal(bits(b[:, :4]), bits(a[:, :4])) and np.array_equal(bits(b[:, CR.ETA]), bits(a[:, CR.ETA]))
        o.set_column(None)
        assert len(o.column) == 0 and _status(mw, o.query_column, q) == mw.MW_ESTATE
    # handles without a column
    with mw.Ocean(resolution=8, length=27.155, wind=(14.45, 12.0), amplitude=0.41, choppiness=0.46, mult=1.5, semantics=mw.MW_SEM_OCEANRENDERER,
                  device=0) as r:
        assert _status(mw, r.set_column, depths) == mw.MW_EINVAL and _status(mw, r.query_column, q) == mw.MW_EINVAL
    with mw.Ocean(resolution=8, length=27.155, wind=(14.45, 12.0), amplitude=0.41, choppiness=0.46, mult=1.5, semantics=mw.MW_SEM_OCEANRENDERER,
                  device=0, ntiles=2) as r:
        assert _status(mw, r.set_column, depths) == mw.MW_EINVAL and _status(mw, r.query_column, q) == mw.MW_EINVAL
        assert _status(mw, r.column_layers, 0) == mw.MW_EINVAL


@pytest.mark.parametrize("change", ["time", "choppiness"])
def test_a_new_frame_gives_the_answers_of_a_fresh_handle(mw, change):
    p = workloads.fftmesh_params(64)
    depths = _depths(4)
    q = np.random.default_rng(4).uniform([-28, -8, -28], [28, 1, 28], (2000, 3)).astype(f32)
    with _ocean(mw, p) as o:
        o.set_column(depths)
        o.evaluate(1.0)
        first = o.query_column(q)
        if change == "choppiness":
            o.set_choppiness(1.2)
            assert np.array_equal(bits(o.query_column(q)), bits(first))     # until the next frame the latest frame's choppiness holds
        o.evaluate(3.5 if change == "time" else 1.0)
        again = o.query_column(q)
    with _ocean(mw, p) as f:
        if change == "choppiness":
            f.set_choppiness(1.2)
        f.evaluate(3.5 if change == "time" else 1.0)
        f.set_column(depths)
        fresh = f.query_column(q)
    assert np.array_equal(bits(again), bits(fresh)) and not np.array_equal(bits(again), bits(first))


# ---- nothing else moves ------------------------------------------------------------------------------------------------------------
def _services(mw, o, t):
    """what every other service returns for one frame"""
    rng = np.random.default_rng(12)
    frame = o.evaluate(t)
    xz = rng.uniform(-28, 28, (500, 2)).astype(f32)
    hull, tris = H.box(3.0, 1.0, 3.0)
    bodies = mw.pack_bodies(np.stack([xz[:16, 0], np.zeros(16), xz[:16, 1]], 1), velocity=rng.standard_normal((16, 3)))
    m, _, I = mw.hull_mass_properties(hull, tris, 500.0)
    mass = mw.pack_mass(np.full(16, m), np.broadcast_to(I, (16, 3, 3)))
    out = [*frame, o.query_surface(xz), o.query_velocity(xz), o.hull_forces(hull, tris, bodies, linear_drag=30.0, quadratic_drag=60.0)]
    stepped, rows = o.step_bodies(hull, tris, bodies.copy(), mass, 0.02, substeps=2, linear_drag=30.0, return_forces=True)
    org = np.stack([xz[:, 0], np.full(500, 20.0), xz[:, 1]], 1)
    rc, hit = o.raycast(org, np.tile([0.1, -1.0, 0.05], (500, 1)))
    return out + [stepped, rows, rc, hit.astype(f32), o.velocity()]


def test_a_column_changes_nothing_another_service_returns(mw):
    p = workloads.fftmesh_params(64, choppiness=1.0)
    q = np.random.default_rng(4).uniform([-28, -8, -28], [28, 1, 28], (3000, 3)).astype(f32)
    with _ocean(mw, p) as plain:
        want = _services(mw, plain, 1.7)
    with _ocean(mw, p) as o:
        o.set_column(_depths(5))
        o.evaluate(0.3)
        o.query_column(q)
        got = _services(mw, o, 1.7)          # a new frame over a built column
        o.query_column(q, mode="rest")
        o.query_column(q)
        again = _services(mw, o, 1.7)        # ... and once more after the column was rebuilt and queried on that frame
    for k, (a, b, c) in enumerate(zip(want, got, again)):
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(c)), k
