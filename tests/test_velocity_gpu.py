"""GPU tier of the surface velocity (mw_ocean_velocity / _device, mw_ocean_query_velocity / _device, include/mistral_water.h) through the
C ABI: field parity with the f64 oracle fed the weighted spectrum (tests/velocity_ref.py) on every evaluation path, consistency with the
library's own frames, the queries against the surface query and numpy, no state change, no stale spectrum, and the error statuses."""
import subprocess
import sys

import numpy as np
import pytest

import surface_ref as S
import velocity_ref as V
import workloads
from conftest import REPO

pytestmark = pytest.mark.gpu


def _ocean(mw, p, seed=1):
    return mw.Ocean(resolution=p.N, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                    choppiness=p.choppiness, gravity=p.gravity, seed=seed, device=0)


def _renderer(mw, res, choppiness=1.5, seed=1):
    return mw.Ocean(resolution=res, unit_width=1.0, length=27.155 * res / 8, wind=(14.45, 12.0), amplitude=0.41, choppiness=choppiness,
                    mult=1.5, seed=seed, semantics=mw.MW_SEM_OCEANRENDERER, device=0)


def _rp(oracle, res, choppiness=1.5):
    return oracle.RendererParams(resolution=res, length=27.155 * res / 8, wind_x=14.45, wind_y=12.0, amplitude=0.41, choppiness=choppiness,
                                 gravity=9.81, mult=1.5)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _assert_field(vel, ref, rel, tag):
    """the scale-relative bound of the position parity tests (workloads.assert_parity): rel * max|field| + 1 ulp of the value"""
    scale = max(float(np.abs(ref).max()), 1e-30)
    err = np.abs(vel - ref)
    bound = rel * scale + np.abs(ref) * 2.0 ** -23
    assert (err <= bound).all(), f"{tag}: max excess {float((err - bound).max()):.3e}, max err / scale {float(err.max()) / scale:.3e}"


FFT_N = [64, 256, 1024, 4096]  # the FFT path starts at 64^2 (use_fft: a power of two >= 64, unit_width == length / N)
# 8^2 and the other non-FFT grids run the chirp-z path: one launch (k_czt_one) up to N = 20, else two or three (asserted below)
DIRECT = [("8", 8, 1.0, 8.0), ("shipped12", 12, 1.0, 12.39), ("50", 50, 1.0, 50.0), ("1000", 1000, 1.0, 1000.0)]


@pytest.mark.parametrize("N", FFT_N)
def test_fftmesh_fft_velocity_matches_oracle(mw, oracle, N):
    p = workloads.fftmesh_params(N)
    with _ocean(mw, p) as o:
        o.evaluate(1.7)
        vel = o.velocity()
        h0, h0c = o.get_spectrum()
    ref = V.fftmesh_velocity_f64(p, h0.reshape(N, N, 2), h0c.reshape(N, N, 2), 1.7)
    _assert_field(vel, ref, workloads.REL_TOL, f"FFT N={N}")


@pytest.mark.parametrize("name,N,u,L", DIRECT, ids=[d[0] for d in DIRECT])
def test_fftmesh_direct_velocity_matches_oracle(mw, oracle, name, N, u, L):
    p = workloads.shipped_fftmesh_scene() if name == "shipped12" else oracle.Params(
        N=N, unit_width=u, length=L, wind_x=14.45, wind_y=12.0, amplitude=1.5e-8 * (1024.0 / N) ** 2 * (L / N) ** 2, choppiness=0.46)
    with _ocean(mw, p) as o:
        assert o.max_batch == 1
        kinds = [k for k, _ in o.profile_kernels(nsteps=1, iters=2)]  # (a frame of its own: the one below replaces it)
        assert "k_czt" in kinds[1] and (("k_czt_one" in kinds[1]) == (N <= 20)), kinds
        o.evaluate(0.75)
        vel = o.velocity()
        h0, h0c = o.get_spectrum()
    ref = V.fftmesh_velocity_f64(p, h0.reshape(N, N, 2), h0c.reshape(N, N, 2), 0.75)
    _assert_field(vel, ref, 2e-5, f"chirp-z N={N}")  # the direct paths' position tolerance (tests/test_gpu_parity.py)


_GEMM_CHILD = r'''
import sys
import numpy as np
sys.path[:0] = [%(repo)r, %(repo)r + "/mistral-water_amd", %(repo)r + "/tests"]
import torch; torch.cuda.is_available()
import mistral_water as mw, velocity_ref as V
from oracle import oracle as O
mw.set_switch("MW_DIRECT_CZT", 0)      # the GEMM form of the separable sum, read when a handle is created
for (N, u, L, amp) in ((12, 1.0, 12.39, 0.01), (65, 0.5, 40.0, 1e-5)):
    p = O.Params(N=N, unit_width=u, length=L, wind_x=5.0, wind_y=3.0, amplitude=amp, choppiness=0.8)
    with mw.Ocean(resolution=N, unit_width=u, length=L, wind=(5.0, 3.0), amplitude=amp, choppiness=0.8) as o:
        o.evaluate(0.5)
        vel = o.velocity()
        h0, h0c = o.get_spectrum()
    ref = V.fftmesh_velocity_f64(p, h0.reshape(N, N, 2), h0c.reshape(N, N, 2), 0.5)
    sc = float(np.abs(ref).max())
    assert (np.abs(vel - ref) <= 2e-5 * sc + np.abs(ref) * 2.0 ** -23).all(), (N, float(np.abs(vel - ref).max()) / sc)
print("GEMM_OK")
'''


def test_fftmesh_gemm_velocity_matches_oracle():
    """the GEMM form of the direct sum (k_direct_spec + k_direct_assemble on the weighted spectrum), in a child with its selector set"""
    r = subprocess.run([sys.executable, "-c", _GEMM_CHILD % {"repo": REPO}], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "GEMM_OK" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.parametrize("res", [8, 64, 128])
def test_renderer_velocity_matches_oracle(mw, oracle, res):
    rp = _rp(oracle, res)
    with _renderer(mw, res) as r:
        for dt in (0.016, 0.033, 0.02):
            r.generate_texture(dt)
        vel = r.velocity()
        init4 = np.concatenate([a.reshape(rp.M, rp.M, 2) for a in r.get_spectrum()], -1)
        phase = r.get_phase().reshape(rp.M, rp.M)
    ref = V.renderer_velocity_f64(rp, init4, phase)
    _assert_field(vel, ref, 4e-6, f"OceanRenderer res={res}")


def test_renderer_velocity_is_the_derivative_of_the_frames(mw, oracle):
    """OceanRenderer resolution 16, mult = 1.5: velocity() at the phase p0 against (displace_mesh after generate_texture(+h) from p0 -
    displace_mesh after generate_texture(-h) from p0) / 2h: the library's own frames, per second of delta_time, mult included (the
    phase advances by w delta_time mult).  The bound is derived, term by term (C = sum (|init.rg| + |init.ba|) max(1, chop) / 8 bounds a
    vertex's sensitivity to its phases, W = w mult):
      the float32 vertices: 2 ulp(max |vertex|) / 2h;
      the frames' transform error: 2 x 4e-6 max |vertex - rest| / 2h (the stated texture tolerance, test_renderer_velocity_matches_oracle);
      the float32 phases of the two frames: <= ulp(2 pi) each, a vertex by <= ulp(2 pi) C, over 2h twice;
      the truncation: h^2 / 6 sum (|init.rg| + |init.ba|) W^3 max(1, chop) / 8;
      the velocity's own error: 4e-6 max |velocity| + 1 ulp."""
    res, h = 16, 2.0 ** -7
    rp = _rp(oracle, res)
    assert rp.mult != 1.0
    with _renderer(mw, res) as r:
        for dt in (0.016, 0.033, 0.02):
            r.generate_texture(dt)
        p0 = r.get_phase()
        vel = r.velocity().astype(np.float64)
        frame = r.displace_mesh()[0].astype(np.float64)  # the latest frame's vertices: the scale of |vertex - rest|
        r.generate_texture(h)
        vp = r.displace_mesh()[0].astype(np.float64)
        r.set_phase(p0)
        r.generate_texture(-h)
        vm = r.displace_mesh()[0].astype(np.float64)
        r.set_phase(p0)
        assert np.array_equal(_bits(r.velocity()), _bits(vel))  # the velocity of a phase does not depend on how the handle got there
        init4 = np.concatenate([a.reshape(rp.M, rp.M, 2) for a in r.get_spectrum()], -1).astype(np.float64)
    rest_plane = S.rest_plane(res, 1.0)
    disp = max(float(np.abs(frame[:, [0, 2]] - rest_plane).max()), float(np.abs(frame[:, 1]).max()))
    W = V.renderer_omega(rp).astype(np.float64) * rp.mult
    C = (np.hypot(init4[..., 0], init4[..., 1]) + np.hypot(init4[..., 2], init4[..., 3])) * max(1.0, rp.choppiness) / 8
    vmax = float(max(np.abs(vp).max(), np.abs(vm).max()))
    scale = float(np.abs(vel).max())
    bound = (2 * float(np.spacing(np.float32(vmax))) / (2 * h) + 2 * 4e-6 * disp / (2 * h)
             + float(np.spacing(np.float32(2 * np.pi))) * float(C.sum()) / h + h * h / 6 * float((C * W ** 3).sum())
             + 4e-6 * scale + float(np.spacing(np.float32(scale))))
    err = np.abs((vp - vm) / (2 * h) - vel)
    assert float(err.max()) <= bound and bound < 0.05 * scale, (float(err.max()), bound, scale)
    # the velocity per unit of delta_time * mult (the weight w alone) is off by the factor mult: far outside the bound
    assert float(np.abs((vp - vm) / (2 * h) - vel / rp.mult).max()) > 10 * bound


def test_query_velocity_refuses_a_surface_behind_the_phase(mw, oracle):
    """query_velocity locates on the latest frame's mesh; after set_phase / advance_phase / set_spectrum without a new frame the velocity
    would belong to another instant: MW_ESTATE until the next frame (mw_ocean_velocity itself answers for the current phase)."""
    xz = np.zeros((3, 2), np.float32)
    with _renderer(mw, 8) as r:
        r.generate_texture(0.02)
        r.query_velocity(xz)
        for move in (lambda: r.advance_phase([0.01]), lambda: r.set_phase(r.get_phase()),
                     lambda: r.set_spectrum(*[a.copy() for a in r.get_spectrum()])):
            move()
            with pytest.raises(mw.MistralWaterError) as e:
                r.query_velocity(xz)
            assert e.value.status == mw.MW_ESTATE and b"different instants" in mw.lib().mw_last_error()
            r.velocity()
            r.generate_texture(0.02)
            r.query_velocity(xz)
    p = workloads.fftmesh_params(64)
    with _ocean(mw, p) as o:
        o.evaluate(1.0)
        o.query_velocity(xz)
        h0, h0c = oracle.generate_spectrum(p, 3)
        o.set_spectrum(h0, h0c)
        with pytest.raises(mw.MistralWaterError) as e:
            o.query_velocity(xz)
        assert e.value.status == mw.MW_ESTATE
        o.evaluate(1.0)
        o.query_velocity(xz)


def test_fftmesh_velocity_is_the_derivative_of_the_frames(mw):
    """256^2: (evaluate(t + h) - evaluate(t - h)) / 2h against velocity(t).  The bound is derived, term by term:
      the float32 vertices: each frame's vertex is rounded (and carries the transform error, far below an ulp of the rest coordinate):
          2 ulp(max |vertex|) / 2h;
      the truncation of the central difference: h^2 max|d^3/dt^3| / 6, max|d^3/dt^3| <= C3 = sum (|h0| + |h0c|) w^3 max(1, chop);
      the float32 phase w t of every frame (S/FFTMesh.cs:183, as the kernels form it): off by <= ulp(w_max (t + h)) / 2 per term, so a
          vertex by <= that times C = sum (|h0| + |h0c|) max(1, chop), twice over 2h."""
    p = workloads.fftmesh_params(256)
    t, h = 3.0, 2.0 ** -6  # t +- h exact in float32
    with _ocean(mw, p) as o:
        vp = o.evaluate(t + h)[0].astype(np.float64)
        vm = o.evaluate(t - h)[0].astype(np.float64)
        o.evaluate(t)
        vel = o.velocity()
        h0, h0c = o.get_spectrum()
    h0, h0c = h0.reshape(-1, 2), h0c.reshape(-1, 2)
    w = V.fftmesh_omega(p).reshape(-1)
    mag = (np.hypot(h0[:, 0], h0[:, 1]) + np.hypot(h0c[:, 0], h0c[:, 1])).astype(np.float64) * max(1.0, p.choppiness)
    vmax = float(max(np.abs(vp).max(), np.abs(vm).max()))
    bound = (2 * float(np.spacing(np.float32(vmax))) / (2 * h) + h * h / 6 * float((mag * w ** 3).sum())
             + float(np.spacing(np.float32(w.max() * (t + h)))) / 2 * float(mag.sum()) / h)
    err = float(np.abs((vp - vm) / (2 * h) - vel).max())
    assert err <= bound and bound < 0.1 * float(np.abs(vel).max()), (err, bound, float(np.abs(vel).max()))


def _world_points(vert, R, uw, n, seed):
    rc = S.rest_coords(R, uw)
    dmax = float(np.abs(vert[:, [0, 2]] - S.rest_plane(R, uw)).max())
    lo, hi = float(rc[0]) + dmax + uw, float(rc[-1]) - dmax - uw
    return np.random.default_rng(seed).uniform(lo, hi, (n, 2)).astype(np.float32)


@pytest.mark.parametrize("sem", ["fftmesh", "renderer"])
def test_query_velocity(mw, sem):
    """rest mode at the vertices: the vertex velocities bit for bit; world mode: residuals bit-identical to query_surface, velocities the
    numpy interpolation at the located point u* (the query is linear in the vertex velocities: u* itself comes from the surface query's
    position through the located triangle); host and device forms bit-identical."""
    import torch
    if sem == "fftmesh":
        p = workloads.fftmesh_params(64, choppiness=1.5)
        ctx = _ocean(mw, p)
    else:
        ctx = _renderer(mw, 32)
    with ctx as o:
        if sem == "fftmesh":
            vert = o.evaluate(1.3)[0]
            R, uw = p.N, p.unit_width
        else:
            o.generate_texture(0.4)
            vert = o.displace_mesh()[0]
            R, uw = 32, 1.0
        vel = o.velocity()
        rest = S.rest_plane(R, uw)
        out = o.query_velocity(rest, mode="rest")
        assert np.array_equal(_bits(out[:, :3]), _bits(vel)) and (out[:, 3] == 0).all()
        xz = _world_points(vert, R, uw, 2000, seed=R)
        qv = o.query_velocity(xz, mode="world", iterations=16)
        qs = o.query_surface(xz, mode="world", iterations=16)
        assert np.array_equal(_bits(qv[:, 3]), _bits(qs[:, 7]))
        # device form, bit-identical
        d_xz = torch.from_numpy(xz).cuda()
        d_out = torch.empty((len(xz), 4), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        o.query_velocity_device(d_xz.data_ptr(), len(xz), d_out.data_ptr(), mode="world", iterations=16)
        o.synchronize()
        assert np.array_equal(_bits(d_out.cpu().numpy()), _bits(qv))
        d_vel = torch.empty((R * R, 3), dtype=torch.float32, device="cuda")
        o.velocity_device(d_vel.data_ptr())
        o.synchronize()
        assert np.array_equal(_bits(d_vel.cpu().numpy()), _bits(vel))
    # numpy: the triangle holding the located displaced position (bit-identical residual => same u*) interpolated in f64
    ok = qs[:, 7] < 1e-3 * uw
    assert ok.mean() > 0.9
    tris = np.asarray(S.grid_triangles(R))
    P = vert[tris][:, :, [0, 2]].astype(np.float64)  # [T, 3, 2]
    e1, e2 = P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    det = e1[:, 0] * e2[:, 1] - e2[:, 0] * e1[:, 1]
    good = np.abs(det) > 1e-12
    done = 0
    for k in np.nonzero(ok)[0][:200]:
        r = qs[k, [0, 2]].astype(np.float64) - P[:, 0]
        a = np.where(good, (r[:, 0] * e2[:, 1] - e2[:, 0] * r[:, 1]) / np.where(good, det, 1), -1)
        b = np.where(good, (e1[:, 0] * r[:, 1] - r[:, 0] * e1[:, 1]) / np.where(good, det, 1), -1)
        wt = np.stack([1 - a - b, a, b], 1)
        inside = (wt >= -1e-4).all(1)
        if not inside.any():
            continue
        y = np.einsum("tk,tk->t", wt[inside], vert[tris[inside], 1])
        j = int(np.argmin(np.abs(y - qs[k, 1])))
        if abs(y[j] - qs[k, 1]) > 1e-4 * max(1.0, float(np.abs(vert[:, 1]).max())):
            continue
        ref = wt[inside][j] @ vel[tris[inside][j]].astype(np.float64)
        np.testing.assert_allclose(qv[k, :3], ref, rtol=1e-6, atol=2e-5 * float(np.abs(vel).max()))  # weights recovered from f32 positions
        done += 1
    assert done >= 100, done


def test_velocity_changes_no_state(mw):
    """frames, timer, phase and surface queries are bit-identical with and without velocity calls in between"""
    p = workloads.fftmesh_params(256)
    xz = S.rest_plane(256, 1.0)[::97] * 0.9

    def fft_run(with_vel):
        out = []
        with _ocean(mw, p) as o:
            for k in range(3):
                v, n, c = o.update(0.03)
                if with_vel:
                    o.velocity(); o.query_velocity(xz, mode="world")
                out += [v, n, c, np.float32(o.timer), o.query_surface(xz, mode="world")]
            if with_vel:
                o.velocity()
            out += [o.evaluate(2.5)[0]]
        return out

    a, b = fft_run(False), fft_run(True)
    assert all(np.array_equal(_bits(np.atleast_1d(x)), _bits(np.atleast_1d(y))) for x, y in zip(a, b))

    def or_run(with_vel):
        out = []
        with _renderer(mw, 16) as r:
            for k in range(3):
                t = r.generate_texture(0.02)
                if with_vel:
                    r.velocity(); r.query_velocity(xz[:10] * 0.05, mode="world")
                out += list(t) + [r.get_phase(), r.query_surface(xz[:10] * 0.05, mode="world")]
            fr = r.generate_texture_steps([0.01, 0.02, 0.03])
            if with_vel:
                r.velocity(frame=2); r.velocity()
            out += list(fr) + [r.get_phase(), r.query_surface(xz[:10] * 0.05, mode="world", frame=1)]
        return out

    a, b = or_run(False), or_run(True)
    assert all(np.array_equal(_bits(x), _bits(y)) for x, y in zip(a, b))


def test_velocity_follows_a_new_spectrum(mw, oracle):
    """after set_spectrum / reinit_spectrum the velocity is that of the new spectrum (the weighted spectrum is rebuilt)"""
    p = workloads.fftmesh_params(64)
    with _ocean(mw, p) as o:
        o.evaluate(1.0)
        v1 = o.velocity()
        h0, h0c = oracle.generate_spectrum(p, 99)
        o.set_spectrum(h0, h0c)
        o.evaluate(1.0)
        v2 = o.velocity()
        ref = V.fftmesh_velocity_f64(p, h0, h0c, 1.0)
        _assert_field(v2, ref, workloads.REL_TOL, "after set_spectrum")
        assert not np.array_equal(v1, v2)
        o.reinit_spectrum(length=p.length, wind=(3.0, -7.0), amplitude=p.amplitude, seed=5)
        o.evaluate(1.0)
        v3 = o.velocity()
        g0, g0c = o.get_spectrum()
        _assert_field(v3, V.fftmesh_velocity_f64(p, g0.reshape(64, 64, 2), g0c.reshape(64, 64, 2), 1.0), workloads.REL_TOL, "after reinit")
    rp = _rp(oracle, 8)
    with _renderer(mw, 8) as r:
        r.generate_texture(0.1)
        w1 = r.velocity()
        init4 = oracle.renderer_initial_spectrum(rp, 42)
        r.set_spectrum(init4[..., :2].copy(), init4[..., 2:].copy())
        r.generate_texture(0.1)
        w2 = r.velocity()
        ref = V.renderer_velocity_f64(rp, init4, r.get_phase().reshape(rp.M, rp.M))
        _assert_field(w2, ref, 4e-6, "renderer after set_spectrum")
        assert not np.array_equal(w1, w2)


def test_velocity_error_statuses(mw):
    import ctypes as C
    L = mw.lib()
    v = np.zeros((64 * 64, 3), np.float32)
    xz = np.zeros((4, 2), np.float32)
    out = np.zeros((4, 4), np.float32)
    p = workloads.fftmesh_params(64)
    _p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    with _ocean(mw, p) as o:
        h = o._h
        assert L.mw_ocean_velocity(h, -1, _p(v)) == mw.MW_ESTATE
        assert L.mw_ocean_query_velocity(h, -1, 1, _p(xz), 4, 0, _p(out)) == mw.MW_ESTATE
        o.evaluate(1.0)
        assert L.mw_ocean_velocity(h, 0, _p(v)) == mw.MW_EINVAL
        assert L.mw_ocean_velocity(h, -1, None) == mw.MW_EINVAL
        assert L.mw_ocean_velocity_device(h, -1, None) == mw.MW_EINVAL
        assert L.mw_ocean_query_velocity(h, -1, 2, _p(xz), 4, 0, _p(out)) == mw.MW_EINVAL
        assert L.mw_ocean_query_velocity(h, -1, 1, _p(xz), 4, 65, _p(out)) == mw.MW_EINVAL
        assert L.mw_ocean_query_velocity(h, -1, 1, None, 4, 0, _p(out)) == mw.MW_EINVAL
        assert L.mw_ocean_query_velocity(h, -1, 1, _p(xz), -1, 0, _p(out)) == mw.MW_EINVAL
        assert L.mw_ocean_query_velocity(h, -1, 1, _p(xz), 2 ** 33, 0, _p(out)) == mw.MW_EINVAL
        assert L.mw_ocean_query_velocity(h, -1, 1, _p(xz), 0, 0, _p(out)) == mw.MW_OK
    with _renderer(mw, 8) as r:
        h = r._h
        assert L.mw_ocean_velocity(h, -1, _p(v)) == mw.MW_ESTATE
        r.generate_texture_steps([0.01, 0.02, 0.03])
        assert L.mw_ocean_velocity(h, 2, _p(v)) == mw.MW_OK
        assert L.mw_ocean_velocity(h, 1, _p(v)) == mw.MW_EINVAL
        assert b"latest phase" in L.mw_last_error()
        r.generate_texture(0.01)
        assert L.mw_ocean_velocity(h, 2, _p(v)) == mw.MW_EINVAL
        assert L.mw_ocean_velocity(h, -1, _p(v)) == mw.MW_OK
    with mw.Ocean(resolution=8, length=27.155, wind=(14.45, 12.0), amplitude=0.41, choppiness=1.5, semantics=mw.MW_SEM_OCEANRENDERER,
                  device=0, ntiles=2) as b:
        b.generate_texture(0.01)
        assert L.mw_ocean_velocity(b._h, -1, _p(v)) == mw.MW_EINVAL
        assert L.mw_ocean_query_velocity(b._h, -1, 1, _p(xz), 4, 0, _p(out)) == mw.MW_EINVAL
