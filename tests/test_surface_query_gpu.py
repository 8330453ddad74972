"""GPU tier of the surface queries (mw_ocean_query_surface / _device, include/mistral_water.h) through the C ABI.

The reference is built from the library's own outputs: the vertices, normals and colours of mw_ocean_evaluate (FFTMesh) or
mw_ocean_displace_mesh (OceanRenderer), the triangles of mw_ocean_rest_mesh, and the float64 brute force of tests/surface_ref.py."""
import numpy as np
import pytest

import surface_ref as S
import workloads

pytestmark = pytest.mark.gpu


def _ocean(mw, p, choppiness=None):
    return mw.Ocean(resolution=p.N, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                    choppiness=p.choppiness if choppiness is None else choppiness, gravity=p.gravity, device=0)


def _renderer(mw, res, choppiness=1.5, seed=1):
    return mw.Ocean(resolution=res, unit_width=1.0, length=27.155 * res / 8, wind=(14.45, 12.0), amplitude=0.41, choppiness=choppiness,
                    mult=1.5, seed=seed, semantics=mw.MW_SEM_OCEANRENDERER, device=0)


def _triangles_match_rest_mesh(o, R):
    idx = o.rest_mesh()[3]
    assert sorted(map(tuple, idx.reshape(-1, 3))) == sorted(map(tuple, S.grid_triangles(R)))


def _world_points(vert, R, uw, n, seed, margin=1.0):
    rc = S.rest_coords(R, uw)
    dmax = float(np.abs(vert[:, [0, 2]] - S.rest_plane(R, uw)).max())
    lo, hi = float(rc[0]) + dmax + margin * uw, float(rc[-1]) - dmax - margin * uw
    if hi <= lo:
        lo, hi = float(rc[0]), float(rc[-1])
    return np.random.default_rng(seed).uniform(lo, hi, (n, 2)).astype(np.float32), dmax


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


FFT_CASES = [("64", lambda: workloads.fftmesh_params(64), 1.5), ("256", lambda: workloads.fftmesh_params(256), 1.0),
             ("shipped12", workloads.shipped_fftmesh_scene, None)]


@pytest.mark.parametrize("name,params,chop", FFT_CASES, ids=[c[0] for c in FFT_CASES])
def test_fftmesh_rest_mode_at_vertices_and_world_mode_against_brute_force(mw, name, params, chop):
    p = params()
    with _ocean(mw, p, chop) as o:
        R, uw = p.N, p.unit_width
        v, n, c = o.evaluate(1.7)
        if R <= 64:
            _triangles_match_rest_mesh(o, R)
        white = c[:, 0].copy()
        rest = S.rest_plane(R, uw)
        out = o.query_surface(rest, mode="rest")
        np.testing.assert_allclose(out[:, :3], v, rtol=1e-6, atol=0)
        np.testing.assert_allclose(out[:, 3:6], n, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(out[:, 6], white, rtol=1e-6, atol=0)
        assert (out[:, 7] == 0).all()
        xz, dmax = _world_points(v, R, uw, 300 if R <= 64 else 150, seed=R)
        w = o.query_surface(xz, mode="world", iterations=16)
        tris_for = S.all_triangles(R) if R <= 64 else S.window_triangles(R, uw, dmax + 2 * uw)
        nuniq, nfold, nmissed = S.check_world(w, xz, v, n, white, uw, tris_for, unique_exact=False)
        assert nuniq >= 0.5 * len(xz) and nmissed <= 0.02 * nuniq, (nuniq, nfold, nmissed)
        # off the footprint in rest mode: NaN, status OK
        assert np.isnan(o.query_surface(np.array([[1e6, 0.0]], np.float32), mode="rest")).all()


def test_fftmesh_1024_world_mode_in_local_windows(mw):
    p = workloads.fftmesh_params(1024)
    with _ocean(mw, p, 1.2) as o:
        v, n, c = o.evaluate(3.25)
        xz, dmax = _world_points(v, 1024, p.unit_width, 200, seed=11)
        w = o.query_surface(xz)
        nuniq, nfold, nmissed = S.check_world(w, xz, v, n, c[:, 0].copy(), p.unit_width, S.window_triangles(1024, p.unit_width, dmax + 2.0),
                                              unique_exact=False)
        assert nuniq >= 0.5 * len(xz) and nmissed <= 0.02 * nuniq, (nuniq, nfold, nmissed)
        idx = np.random.default_rng(5).integers(0, 1024 * 1024, 4096)
        r = o.query_surface(S.rest_plane(1024, p.unit_width)[idx], mode="rest")
        np.testing.assert_allclose(r[:, :3], v[idx], rtol=1e-6, atol=0)


@pytest.mark.parametrize("res", [8, 128])
def test_oceanrenderer_rest_mode_at_vertices_and_world_mode_against_brute_force(mw, res):
    with _renderer(mw, res) as o:
        for dt in (0.016, 0.5, 0.033):
            o.generate_texture(dt)
        v, n, c = o.displace_mesh()
        if res == 8:
            _triangles_match_rest_mesh(o, res)
        out = o.query_surface(S.rest_plane(res, 1.0), mode="rest")
        np.testing.assert_allclose(out[:, :3], v, rtol=1e-6, atol=0)
        np.testing.assert_allclose(out[:, 3:6], n, rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(out[:, 6], c, rtol=1e-6, atol=0)
        xz, dmax = _world_points(v, res, 1.0, 300, seed=res, margin=0.0)
        w = o.query_surface(xz, mode="world")
        nuniq, nfold, nmissed = S.check_world(w, xz, v, n, c, 1.0, S.all_triangles(res), unique_exact=False)
        assert nuniq >= 0.5 * len(xz) and nmissed <= 0.02 * nuniq, (nuniq, nfold, nmissed)


def test_oceanrenderer_frames_of_a_steps_call_equal_frames_generated_one_by_one(mw):
    dts = [0.016, 0.4, 0.033, 0.25]
    with _renderer(mw, 16, seed=9) as a, _renderer(mw, 16, seed=9) as b:
        a.generate_texture_steps(dts)
        xz = np.random.default_rng(1).uniform(-9.0, 9.0, (2000, 2)).astype(np.float32)
        for k, dt in enumerate(dts):
            b.generate_texture(dt)
            for mode in ("world", "rest"):
                fa = a.query_surface(xz, mode=mode, frame=k)
                fb = b.query_surface(xz, mode=mode, frame=-1)
                assert np.array_equal(_bits(fa), _bits(fb)), (k, mode)
        assert np.array_equal(_bits(a.query_surface(xz, frame=-1)), _bits(a.query_surface(xz, frame=3)))


def test_host_and_device_forms_are_bit_identical(mw):
    import torch
    rng = np.random.default_rng(3)
    with _ocean(mw, workloads.fftmesh_params(256), 1.0) as o, _renderer(mw, 32) as r:
        o.evaluate(2.0)
        r.generate_texture_steps([0.02, 0.3])
        for h, frame in ((o, -1), (r, 0), (r, 1), (r, -1)):
            xz = rng.uniform(-140.0, 140.0, (100003, 2)).astype(np.float32)
            for mode in ("world", "rest"):
                host = h.query_surface(xz, mode=mode, frame=frame, iterations=12)
                d_xz = torch.from_numpy(xz).cuda()
                d_out = torch.full((len(xz), 8), 7.0, device="cuda")
                torch.cuda.synchronize()
                h.query_surface_device(d_xz.data_ptr(), len(xz), d_out.data_ptr(), mode=mode, frame=frame, iterations=12)
                h.synchronize()
                assert np.array_equal(_bits(host), _bits(d_out.cpu().numpy())), (frame, mode)


def test_queries_change_no_later_output(mw):
    xz = np.random.default_rng(4).uniform(-60.0, 60.0, (5000, 2)).astype(np.float32)
    p = workloads.fftmesh_params(128)
    with _ocean(mw, p) as a, _ocean(mw, p) as b:
        a.evaluate(1.0); b.evaluate(1.0)
        a.query_surface(xz); a.query_surface(xz, mode="rest")
        for x, y in zip(a.evaluate(2.5), b.evaluate(2.5)):
            assert np.array_equal(_bits(x), _bits(y))
        assert np.array_equal(_bits(a.query_surface(xz)), _bits(b.query_surface(xz)))
    with _renderer(mw, 16, seed=2) as a, _renderer(mw, 16, seed=2) as b:
        a.generate_texture(0.02); b.generate_texture(0.02)
        a.generate_texture_steps([0.1, 0.2]); b.generate_texture_steps([0.1, 0.2])
        a.query_surface(xz); a.query_surface(xz, frame=0, mode="rest")
        for x, y in zip(a.displace_mesh(), b.displace_mesh()):
            assert np.array_equal(_bits(x), _bits(y))
        for x, y in zip(a.generate_texture(0.05), b.generate_texture(0.05)):
            assert np.array_equal(_bits(x), _bits(y))
        assert np.array_equal(_bits(a.get_phase()), _bits(b.get_phase()))


def test_query_statuses_on_real_handles(mw):
    L = mw.lib()
    xz = np.zeros((4, 2), np.float32)
    out = np.zeros((4, 8), np.float32)

    def st(o, frame=-1, mode=1, n=4, iters=0, a=xz, b=out):
        return L.mw_ocean_query_surface(o.handle, frame, mode, None if a is None else a.ctypes.data, n, iters,
                                        None if b is None else b.ctypes.data)
    with _ocean(mw, workloads.fftmesh_params(64)) as o:
        assert st(o) == mw.MW_ESTATE                       # no frame yet
        o.evaluate(1.0)
        assert st(o) == mw.MW_OK and st(o, n=0, a=None, b=None) == mw.MW_OK
        assert st(o, frame=0) == mw.MW_EINVAL and st(o, mode=2) == mw.MW_EINVAL
        assert st(o, iters=65) == mw.MW_EINVAL and st(o, iters=-1) == mw.MW_EINVAL and st(o, iters=64) == mw.MW_OK
        assert st(o, n=-1) == mw.MW_EINVAL and st(o, a=None) == mw.MW_EINVAL and st(o, b=None) == mw.MW_EINVAL
        assert st(o, n=2 ** 32) == mw.MW_EINVAL           # more than one launch holds: refused before any array is read
    with _ocean(mw, workloads.shipped_fftmesh_scene()) as o:
        o.profile_kernels(1, 2)                            # the chirp-z path writes the host-API frame too
        assert st(o) == mw.MW_OK
    with _renderer(mw, 8) as r:
        assert st(r) == mw.MW_ESTATE
        assert st(r, frame=0) == mw.MW_EINVAL             # no steps call yet
        r.generate_texture_steps([0.1, 0.2, 0.3])
        assert st(r) == mw.MW_OK and st(r, frame=2) == mw.MW_OK
        assert st(r, frame=3) == mw.MW_EINVAL and st(r, frame=-2) == mw.MW_EINVAL
    with mw.Ocean(resolution=8, length=27.155, wind=(14.45, 12.0), amplitude=0.41, choppiness=0.46, mult=1.5,
                  semantics=mw.MW_SEM_OCEANRENDERER, device=0, ntiles=2) as t:
        t.generate_texture(0.1)
        assert st(t) == mw.MW_EINVAL                      # batched handles: out of scope


@pytest.mark.parametrize("name,params,t", [
    ("fft64", lambda: workloads.fftmesh_params(64, choppiness=1.5), 1.0),                       # profiled step: t = 1
    ("shipped12", workloads.shipped_fftmesh_scene, float(np.float32(1) + np.float32(1) / np.float32(60)))])  # last of 2 iterations
def test_query_after_the_profiling_hook_reads_its_scalar_whitecap(mw, name, params, t):
    """mw_ocean_profile_kernels(nsteps = 1) leaves its step in the host-API frame with the whitecap as ONE float per vertex (the
    host API writes RGBA colours, four): the query must read it with the stride of the latest writer.  Reference: a second handle
    evaluated at the profiled time."""
    p = params()
    with _ocean(mw, p) as a, _ocean(mw, p) as b:
        a.evaluate(0.3)                                   # an RGBA frame first: a wrong stride would read stale colours
        a.profile_kernels(1, 2)
        v, n, c = b.evaluate(t)
        out = a.query_surface(S.rest_plane(p.N, p.unit_width), mode="rest")
        white = c[:, 0]
        if name == "fft64":
            assert white.max() > white.min()              # a varying whitecap: a wrong stride cannot pass by accident
        np.testing.assert_allclose(out[:, :3], v, rtol=1e-6, atol=1e-6 * float(np.abs(v).max()))
        np.testing.assert_allclose(out[:, 6], white, rtol=1e-6, atol=1e-6 * max(float(np.abs(white).max()), 1e-30))
        a.evaluate(t)                                     # back to the RGBA layout
        out2 = a.query_surface(S.rest_plane(p.N, p.unit_width), mode="rest")
        np.testing.assert_allclose(out2[:, 6], white, rtol=1e-6, atol=1e-6 * max(float(np.abs(white).max()), 1e-30))
