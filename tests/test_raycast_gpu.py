"""GPU tier of the raycasts (mw_ocean_raycast / _device, include/mistral_water.h) through the C ABI.

The reference is the g++ build of the same MW_HD functions (tests/raycast_shim.cpp) run on the library's own vertex arrays: the
vertices, normals and colours of mw_ocean_evaluate (FFTMesh) or mw_ocean_displace_mesh (OceanRenderer).  Every row must match it bit for
bit.  Also: host and device forms, frames of a steps call, the leaf size (switch MW_RC_BLOCK), no state change, the statuses."""
import numpy as np
import pytest

import ray_ref as RR
import workloads

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return RR.build_shim(str(tmp_path_factory.mktemp("rcg") / "librc_shim.so"))


def _ocean(mw, p, choppiness=None):
    return mw.Ocean(resolution=p.N, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                    choppiness=p.choppiness if choppiness is None else choppiness, gravity=p.gravity, device=0)


def _renderer(mw, res, choppiness=1.5, seed=1):
    return mw.Ocean(resolution=res, unit_width=1.0, length=27.155 * res / 8, wind=(14.45, 12.0), amplitude=0.41, choppiness=choppiness,
                    mult=1.5, seed=seed, semantics=mw.MW_SEM_OCEANRENDERER, device=0)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _cast(o, rays, frame=-1):
    return o.raycast(rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7], frame=frame)


def _rays(vert, R, seed, n):
    return np.concatenate(list(RR.families(vert, R, np.random.default_rng(seed), n=n).values()))


def _assert_same(out, hit, so, sh, what=""):
    bad = ~((_bits(out) == _bits(so)).all(1) & (hit == sh).all(1))
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:6], out[bad][:3], so[bad][:3], hit[bad][:3], sh[bad][:3])


FFT_CASES = [("64", lambda: workloads.fftmesh_params(64), 1.5), ("256", lambda: workloads.fftmesh_params(256), 1.0),
             ("shipped12", workloads.shipped_fftmesh_scene, None)]


@pytest.mark.parametrize("name,params,chop", FFT_CASES, ids=[c[0] for c in FFT_CASES])
def test_fftmesh_gpu_equals_the_shim_bit_for_bit(mw, shim, name, params, chop):
    p = params()
    with _ocean(mw, p, chop) as o:
        v, n, c = o.evaluate(1.7)
        m = RR.Mesh(p.N, v, n, c.reshape(-1), wstride=4, uw=p.unit_width)
        rays = _rays(m.vert, p.N, p.N, 300)
        out, hit = _cast(o, rays)
        so, sh = RR.cast(shim, m, rays)
        _assert_same(out, hit, so, sh, name)
        if p.N <= 64:
            bo, bh = RR.cast(shim, m, rays, brute=True)
            _assert_same(out, hit, bo, bh, name + " brute force")
        assert (hit[:, 0] >= 0).mean() > 0.2


def test_fftmesh_1024_against_the_shim(mw, shim):
    """The 1024^2 FFTMesh (leaf level 9: both build launches): a sample of every family against the shim's traversal, and a
    smaller subset against the shim's brute force over all 2 million triangles."""
    p = workloads.fftmesh_params(1024)
    with _ocean(mw, p, 1.2) as o:
        v, n, c = o.evaluate(3.25)
        m = RR.Mesh(1024, v, n, c.reshape(-1), wstride=4)
        rays = _rays(m.vert, 1024, 11, 1500)
        out, hit = _cast(o, rays)
        so, sh = RR.cast(shim, m, rays)
        _assert_same(out, hit, so, sh, "1024 traversal")
        sub = np.random.default_rng(12).choice(len(rays), 48, replace=False)
        bo, bh = RR.cast(shim, m, rays[sub], brute=True)
        _assert_same(out[sub], hit[sub], bo, bh, "1024 brute force")
        assert (hit[:, 0] >= 0).mean() > 0.2


def test_oceanrenderer_gpu_equals_the_shim_bit_for_bit(mw, shim):
    with _renderer(mw, 128) as o:
        for dt in (0.016, 0.5, 0.033):
            o.generate_texture(dt)
        v, n, c = o.displace_mesh()
        m = RR.Mesh(128, v, n, c, wstride=1)
        rays = _rays(m.vert, 128, 128, 300)
        out, hit = _cast(o, rays)
        so, sh = RR.cast(shim, m, rays)
        _assert_same(out, hit, so, sh, "renderer 128")
        sub = slice(0, 400)
        bo, bh = RR.cast(shim, m, rays[sub], brute=True)
        _assert_same(out[sub], hit[sub], bo, bh, "renderer 128 brute force")


def test_the_first_hit_does_not_depend_on_the_leaf_size(mw):
    """The hierarchy is an acceleration structure only: leaf blocks of 1 to 64 cells (switch MW_RC_BLOCK) give the default's bits."""
    p = workloads.fftmesh_params(256)
    with _ocean(mw, p, 1.5) as o:
        v, _, _ = o.evaluate(0.9)
        rays = _rays(v, 256, 3, 200)
        ref = _cast(o, rays)
        try:
            for B in (1, 2, 5, 16, 64):
                mw.set_switch("MW_RC_BLOCK", B)
                out, hit = _cast(o, rays)
                _assert_same(out, hit, *ref, what=B)
        finally:
            mw.set_switch("MW_RC_BLOCK", 0)


def test_host_and_device_forms_are_bit_identical(mw):
    import torch
    with _ocean(mw, workloads.fftmesh_params(256), 1.0) as o, _renderer(mw, 32) as r:
        o.evaluate(2.0)
        r.generate_texture_steps([0.02, 0.3])
        for h, frame, R in ((o, -1, 256), (r, 0, 32), (r, 1, 32), (r, -1, 32)):
            v = h.evaluate(2.0)[0] if h is o else r.displace_mesh()[0]
            rays = _rays(v, R, 5 + frame, 2000)
            out, hit = _cast(h, rays, frame)
            d_rays = torch.from_numpy(rays).cuda()
            d_out = torch.full((len(rays), 8), 7.0, device="cuda")
            d_hit = torch.full((len(rays), 2), 7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            h.raycast_device(d_rays.data_ptr(), len(rays), d_out.data_ptr(), d_hit.data_ptr(), frame=frame)
            h.synchronize()
            _assert_same(d_out.cpu().numpy(), d_hit.cpu().numpy(), out, hit, ("device", frame))
            d_out.fill_(7.0)
            torch.cuda.synchronize()
            h.raycast_device(d_rays.data_ptr(), len(rays), d_out.data_ptr(), 0, frame=frame)   # no hit array
            h.synchronize()
            assert np.array_equal(_bits(d_out.cpu().numpy()), _bits(out)), frame


def test_oceanrenderer_frames_of_a_steps_call_equal_frames_generated_one_by_one(mw):
    dts = [0.016, 0.4, 0.033, 0.25]
    with _renderer(mw, 16, seed=9) as a, _renderer(mw, 16, seed=9) as b:
        a.generate_texture_steps(dts)
        rng = np.random.default_rng(1)
        o = rng.uniform([-10, -3, -10], [10, 6, 10], (3000, 3))
        rays = RR.pack(o, rng.normal(size=(3000, 3)))
        for k, dt in enumerate(dts):
            b.generate_texture(dt)
            _assert_same(*_cast(a, rays, k), *_cast(b, rays, -1), what=k)
        _assert_same(*_cast(a, rays, -1), *_cast(a, rays, 3), what="latest")


def test_raycasts_change_no_later_output(mw):
    rng = np.random.default_rng(4)
    rays = RR.pack(rng.uniform([-60, -5, -60], [60, 20, 60], (5000, 3)), rng.normal(size=(5000, 3)))
    p = workloads.fftmesh_params(128)
    with _ocean(mw, p) as a, _ocean(mw, p) as b:
        a.evaluate(1.0); b.evaluate(1.0)
        _cast(a, rays)
        for x, y in zip(a.evaluate(2.5), b.evaluate(2.5)):
            assert np.array_equal(_bits(x), _bits(y))
        _assert_same(*_cast(a, rays), *_cast(b, rays))
        assert np.array_equal(_bits(a.query_surface(rays[:, [0, 2]])), _bits(b.query_surface(rays[:, [0, 2]])))
    with _renderer(mw, 16, seed=2) as a, _renderer(mw, 16, seed=2) as b:
        a.generate_texture(0.02); b.generate_texture(0.02)
        a.generate_texture_steps([0.1, 0.2]); b.generate_texture_steps([0.1, 0.2])
        _cast(a, rays); _cast(a, rays, 0)
        for x, y in zip(a.displace_mesh(), b.displace_mesh()):
            assert np.array_equal(_bits(x), _bits(y))
        for x, y in zip(a.generate_texture(0.05), b.generate_texture(0.05)):
            assert np.array_equal(_bits(x), _bits(y))
        assert np.array_equal(_bits(a.get_phase()), _bits(b.get_phase()))


def test_raycast_statuses_on_real_handles(mw):
    import torch
    L = mw.lib()
    rays = RR.pack(np.zeros((4, 3)), [0.0, -1.0, 0.0])
    out = np.zeros((4, 8), np.float32)
    hit = np.zeros((4, 2), np.int32)

    def st(o, frame=-1, n=4, a=rays, b=out, h=hit):
        return L.mw_ocean_raycast(o.handle, frame, None if a is None else a.ctypes.data, n, None if b is None else b.ctypes.data,
                                  None if h is None else h.ctypes.data)
    with _ocean(mw, workloads.fftmesh_params(64)) as o:
        assert st(o) == mw.MW_ESTATE                          # no frame yet
        o.evaluate(1.0)
        assert st(o) == mw.MW_OK and st(o, h=None) == mw.MW_OK and st(o, n=0, a=None, b=None, h=None) == mw.MW_OK
        assert st(o, frame=0) == mw.MW_EINVAL
        assert st(o, n=-1) == mw.MW_EINVAL and st(o, a=None) == mw.MW_EINVAL and st(o, b=None) == mw.MW_EINVAL
        assert st(o, n=2 ** 32) == mw.MW_EINVAL              # more than one launch holds: refused before any array is read
        d = torch.zeros(64, device="cuda")
        p0 = d.data_ptr()
        dev = L.mw_ocean_raycast_device
        assert dev(o.handle, -1, p0, 1, p0 + 64, p0 + 128) == mw.MW_OK
        assert dev(o.handle, -1, p0 + 4, 1, p0 + 64, p0 + 128) == mw.MW_EINVAL    # d_rays not 16-byte aligned
        assert dev(o.handle, -1, p0, 1, p0 + 72, p0 + 128) == mw.MW_EINVAL        # d_out not 16-byte aligned
        assert dev(o.handle, -1, p0, 1, p0 + 64, p0 + 132) == mw.MW_EINVAL        # d_hit not 8-byte aligned
        o.synchronize()
    with _ocean(mw, workloads.shipped_fftmesh_scene()) as o:
        o.profile_kernels(1, 2)                                # the chirp-z path writes the host-API frame too
        assert st(o) == mw.MW_OK
    with _renderer(mw, 8) as r:
        assert st(r) == mw.MW_ESTATE
        assert st(r, frame=0) == mw.MW_EINVAL                 # no steps call yet
        r.generate_texture_steps([0.1, 0.2, 0.3])
        assert st(r) == mw.MW_OK and st(r, frame=2) == mw.MW_OK
        assert st(r, frame=3) == mw.MW_EINVAL and st(r, frame=-2) == mw.MW_EINVAL
    with mw.Ocean(resolution=8, length=27.155, wind=(14.45, 12.0), amplitude=0.41, choppiness=0.46, mult=1.5,
                  semantics=mw.MW_SEM_OCEANRENDERER, device=0, ntiles=2) as t:
        t.generate_texture(0.1)
        assert st(t) == mw.MW_EINVAL                         # batched handles: out of scope
