"""CPU tier of the floating bodies (mw_hull_mass_properties, mw_ocean_step_bodies / _device, include/mistral_water.h).

* mass properties through the library (host arrays, no device needed) and through tests/body_ref.py (numpy float64): an axis-aligned
  box against m/12 (b^2 + c^2, ...), an offset box (centroid), a box rotated 30 degrees (R I R^T, signs of the off-diagonal entries), an
  icosphere against hull_ref.volume, and MW_EINVAL for an inward-wound mesh or a bad index;
* the integration step of csrc/rigid_bodies.h through tests/bodies_shim.cpp (g++, strict float32) against body_ref.step for random
  states, forces and inertia tensors, the NaN-row rule and the mass-row check;
* the new entry points, constants and the switch are exported, declared and bound."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import body_ref as B
import hull_ref as H
import shim_build
from conftest import REPO

SHIM = os.path.join(REPO, "tests", "bodies_shim.cpp")
HDR = os.path.join(REPO, "mistral-water_amd", "csrc", "rigid_bodies.h")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def bs(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("bodies") / "libbodies_shim.so")
    L = shim_build.strict_f32(SHIM, path)
    L.bs_integrate.restype = None
    L.bs_integrate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p]
    L.bs_mass_valid.restype = None
    L.bs_mass_valid.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return L


def _rot(axis, deg):
    a = np.radians(deg)
    c, s = np.cos(a), np.sin(a)
    if axis == "x":
        return np.array([[1, 0, 0], [0, c, -s], [0, s, c]])
    if axis == "y":
        return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]])
    return np.array([[c, -s, 0], [s, c, 0], [0, 0, 1]])


def _check_props(mw, x, tris, density, m_exp, c_exp, I_exp, rtol=2e-6):
    m, c, I = mw.hull_mass_properties(x, tris, density)
    rm, rc, rI = B.mass_properties(x, tris, density)
    scale = np.abs(I_exp).max()
    for mm, cc, II in ((m, c, I), (rm, rc, rI)):
        assert abs(mm - m_exp) <= rtol * m_exp
        assert np.abs(cc - c_exp).max() <= rtol * (1 + np.abs(c_exp).max())
        assert np.abs(II - I_exp).max() <= 4 * rtol * scale, (II, I_exp)
    return m, c, I


def test_box_mass_properties(mw):
    a, b, c, rho = 2.0, 0.8, 3.0, 640.0
    x, t = H.box(a, b, c)
    m = rho * a * b * c
    _, _, I = _check_props(mw, x, t, rho, m, np.zeros(3), B.box_inertia(m, a, b, c))
    assert (I[[0, 0, 1], [1, 2, 2]] == 0).all() or np.abs(I[[0, 0, 1], [1, 2, 2]]).max() <= 1e-6 * np.abs(I).max()


def test_offset_box_centroid(mw):
    x, t = H.box(1.5, 1.0, 0.5)
    off = np.array([3.0, -2.0, 7.5], np.float32)
    m = 1000.0 * 0.75
    _check_props(mw, x + off, t, 1000.0, m, off, B.box_inertia(m, 1.5, 1.0, 0.5))


def test_rotated_box_tensor(mw):
    """a box rotated 30 degrees about z and then x: R I0 R^T, with the off-diagonal entries' signs (Ixy = -int xy dm)"""
    w, h, l, rho = 3.0, 1.0, 2.0, 500.0
    x, t = H.box(w, h, l)
    R = _rot("x", 20.0) @ _rot("z", 30.0)
    xr = (x.astype(np.float64) @ R.T).astype(np.float32)
    m = rho * w * h * l
    I0 = B.box_inertia(m, w, h, l)
    _, _, I = _check_props(mw, xr, t, rho, m, np.zeros(3), R @ I0 @ R.T)
    # about z alone by 30 degrees: the long x side turns towards +y, so int xy dm > 0 and Ixy < 0
    xz = (x.astype(np.float64) @ _rot("z", 30.0).T).astype(np.float32)
    _, _, Iz = mw.hull_mass_properties(xz, t, rho)
    assert Iz[0, 1] < 0 and abs(Iz[0, 2]) <= 1e-5 * np.abs(Iz).max() and abs(Iz[1, 2]) <= 1e-5 * np.abs(Iz).max()
    xy = (x.astype(np.float64) @ _rot("z", -30.0).T).astype(np.float32)
    assert mw.hull_mass_properties(xy, t, rho)[2][0, 1] > 0


def test_icosphere_mass_properties(mw):
    x, t = H.icosphere(1.3, 3)
    V = H.volume(x, t)
    m, c, I = mw.hull_mass_properties(x, t, 1000.0)
    assert abs(m - 1000.0 * V) <= 2e-6 * 1000.0 * V
    assert np.abs(c).max() <= 1e-6
    # nearly a solid sphere: 2/5 m r^2 on the diagonal, to the mesh's faceting
    assert np.abs(np.diag(I) - 0.4 * m * 1.3 ** 2).max() <= 0.03 * 0.4 * m * 1.3 ** 2
    rm, rc, rI = B.mass_properties(x, t, 1000.0)
    assert abs(m - rm) <= 2e-6 * rm and np.abs(I - rI).max() <= 1e-5 * np.abs(rI).max()


def test_bad_meshes_are_einval(mw):
    L = mw.lib()
    x, t = H.box(1.0, 1.0, 1.0)
    out = np.full(10, 7.0, np.float32)
    inward = np.ascontiguousarray(t[:, [0, 2, 1]])
    assert L.mw_hull_mass_properties(_p(x), len(x), _p(inward), len(inward), C.c_float(1000.0), _p(out)) == mw.MW_EINVAL
    assert b"volume" in L.mw_last_error()
    bad = t.copy()
    bad[2, 1] = 8
    assert L.mw_hull_mass_properties(_p(x), len(x), _p(bad), len(bad), C.c_float(1000.0), _p(out)) == mw.MW_EINVAL
    assert L.mw_hull_mass_properties(_p(x), len(x), _p(t), len(t), C.c_float(0.0), _p(out)) == mw.MW_EINVAL
    assert L.mw_hull_mass_properties(_p(x), len(x), _p(t), len(t), C.c_float(float("nan")), _p(out)) == mw.MW_EINVAL
    assert L.mw_hull_mass_properties(None, len(x), _p(t), len(t), C.c_float(1.0), _p(out)) == mw.MW_EINVAL
    assert L.mw_hull_mass_properties(_p(x), 2, _p(t), len(t), C.c_float(1.0), _p(out)) == mw.MW_EINVAL
    assert (out == 7.0).all()
    with pytest.raises(mw.MistralWaterError):
        mw.hull_mass_properties(x, inward, 1000.0)


def test_pack_mass(mw):
    I = np.array([[2.0, -0.1, 0.2], [-0.1, 3.0, -0.3], [0.2, -0.3, 4.0]])
    rows = mw.pack_mass([5.0, 6.0], I)
    assert rows.shape == (2, 8) and rows.dtype == np.float32
    assert (rows[:, 1:7] == np.float32([2.0, 3.0, 4.0, -0.1, 0.2, -0.3])).all() and (rows[:, 0] == [5.0, 6.0]).all()
    assert (rows[:, 7] == 0).all()
    assert np.allclose(B.inertia_matrix(rows[0]), I.astype(np.float32))


def _random_spd(rng, n):
    out = []
    for _ in range(n):
        A = rng.standard_normal((3, 3))
        out.append(A @ A.T + 0.5 * np.eye(3))
    return np.array(out)


def test_integration_step_against_reference(mw, bs):
    rng = np.random.default_rng(11)
    n = 400
    bodies = mw.pack_bodies(rng.standard_normal((n, 3)) * 5, H.random_quaternions(n, rng), rng.standard_normal((n, 3)) * 2,
                            rng.standard_normal((n, 3)))
    bodies[:, [3, 11, 15]] = rng.standard_normal((n, 3)).astype(np.float32)  # spare floats pass through
    masses = rng.uniform(0.5, 50.0, n)
    mass = mw.pack_mass(masses, _random_spd(rng, n) * masses[:, None, None])
    rows = np.zeros((n, 8), np.float32)
    rows[:, 0:3] = rng.standard_normal((n, 3)) * masses[:, None] * 5
    rows[:, 3] = rng.uniform(0, 10, n)
    rows[:, 4:7] = rng.standard_normal((n, 3)) * masses[:, None] * 2
    rows[:, 7] = rng.uniform(0, 1e-5, n)
    rows[7] = np.nan  # a NaN row: the body stays
    g, h = 9.81, 1.0 / 120
    out = bodies.copy()
    ok = np.zeros(n, np.int32)
    bs.bs_integrate(_p(out), _p(rows), _p(mass), n, g, h, _p(ok))
    assert ok[7] == 0 and np.array_equal(out[7].view(np.uint32), bodies[7].view(np.uint32))
    for b in range(n):
        if b == 7:
            continue
        assert ok[b] == 1
        ref = B.step(bodies[b], rows[b], mass[b].astype(np.float64), g, h)
        assert np.array_equal(out[b, [3, 11, 15]], bodies[b, [3, 11, 15]])
        for sl in (slice(0, 3), slice(4, 8), slice(8, 11), slice(12, 15)):
            scale = 1.0 + np.abs(ref[sl]).max()
            assert np.abs(out[b, sl] - ref[sl]).max() <= 4e-6 * scale, (b, sl, out[b, sl], ref[sl])
        assert abs(np.linalg.norm(out[b, 4:8].astype(np.float64)) - 1) <= 1e-6


def test_free_fall_and_spin_steps(mw, bs):
    """zero rows: v falls by h g per step, p by h v; a spin about a principal axis turns by 2 atan(h |w| / 2) per step"""
    body = mw.pack_bodies([[0.0, 5.0, 0.0]], velocity=[[1.0, 0.5, 0.0]], angular_velocity=[[0.0, 3.0, 0.0]])
    mass = mw.pack_mass(2.0, np.diag([1.0, 2.0, 3.0]))
    rows = np.zeros((1, 8), np.float32)
    ok = np.zeros(1, np.int32)
    h, K = 0.01, 50
    b = body.copy()
    for _ in range(K):
        bs.bs_integrate(_p(b), _p(rows), _p(mass), 1, 9.81, h, _p(ok))
    assert abs(b[0, 9] - (0.5 - K * h * 9.81)) <= 1e-5
    assert abs(b[0, 1] - (5.0 + K * h * 0.5 - h * h * 9.81 * K * (K + 1) / 2)) <= 1e-5
    angle = 2 * np.arctan2(np.linalg.norm(b[0, 4:7]), b[0, 7])
    assert abs(angle - 2 * K * np.arctan(h * 3.0 / 2)) <= 1e-5 and abs(b[0, 13] - 3.0) <= 1e-6


def test_mass_row_check(bs):
    good = [1.0, 2.0, 3.0, 4.0, 0.1, -0.2, 0.3, 0.0]
    rows = np.array([good,
                     [0.0] + good[1:], [-1.0] + good[1:], [np.inf] + good[1:], [np.nan] + good[1:],
                     [1.0, -2.0, 3.0, 4.0, 0, 0, 0, 0],         # Ixx <= 0
                     [1.0, 1.0, 1.0, 4.0, 2.0, 0, 0, 0],         # 2x2 minor < 0
                     [1.0, 1.0, 1.0, 1.0, 0.9, 0.9, -0.9, 0],    # det < 0 with positive 2x2 minor
                     [1.0, 2.0, np.nan, 4.0, 0, 0, 0, 0],
                     [1.0, 2.0, 3.0, 4.0, np.inf, 0, 0, 0]], np.float32)
    ok = np.zeros(len(rows), np.int32)
    bs.bs_mass_valid(_p(rows), len(rows), _p(ok))
    assert list(ok) == [1] + [0] * (len(rows) - 1)


def test_entry_points_exported_and_bound(mw):
    from mistral_water import _native
    L = mw.lib()
    hdr = open(os.path.join(REPO, "include", "mistral_water.h")).read()
    for s in ("mw_hull_mass_properties", "mw_ocean_step_bodies", "mw_ocean_step_bodies_device"):
        assert hasattr(L, s) and s in _native.ABI_SYMBOLS and s + "(" in hdr
    assert int(re.search(r"#define\s+MW_BODY_NMASS\s+(\d+)", hdr).group(1)) == _native.MW_BODY_NMASS == mw.MW_BODY_NMASS == 8
    cs = open(os.path.join(REPO, "bindings", "csharp", "MistralWaterNative.cs")).read()
    assert int(re.search(r"BodyNMass\s*=\s*(\d+)", cs).group(1)) == 8
    assert mw.get_switch("MW_BODIES_PLAN") == -1


def test_step_bodies_bad_arguments_are_statuses(mw):
    L = mw.lib()
    x, t = H.box(1.0, 1.0, 1.0)
    bodies = mw.pack_bodies([[0.0, 0.0, 0.0]])
    mass = mw.pack_mass(500.0, B.box_inertia(500.0, 1, 1, 1))
    cf = np.array([1000.0, 9.81, 0, 0, 1], np.float32)
    before = bodies.copy()
    for fn in (L.mw_ocean_step_bodies, L.mw_ocean_step_bodies_device):
        assert fn(None, -1, _p(x), 8, _p(t), 12, _p(bodies), _p(mass), 1, _p(cf), C.c_float(0.1), 1, 0, None) == mw.MW_EINVAL
    assert np.array_equal(bodies, before)


def test_kernels_use_the_hd_functions():
    """both plans integrate with body_integrate and sum with the hull-forces functions; the one-launch kernels of a single hull and of a
    fleet call the same ordered sums; the summation order has one definition; nothing between workgroups"""
    src = open(HDR).read()
    csrc = os.path.dirname(HDR)
    hull, fleet = open(os.path.join(csrc, "hull_forces.h")).read(), open(os.path.join(csrc, "fleet.h")).read()
    step = src[src.index("void k_bodies_step"):]
    assert "hull_vertex(ha.m, ha.vel, ha.vscale, ha.iters, body, h, sl)" in step
    assert "hull_triangle(idx, ha.nverts, vs, body, ha.cf, acc)" in step
    assert "hull_row(acc, res, row)" in step and "body_integrate(body, row, mass, a.g, a.dt)" in step
    integ = src[src.index("void k_bodies_integrate"):src.index("void k_bodies_step")]
    assert "body_integrate(body, row, mass, a.g, a.dt)" in integ
    # the two one-launch kernels sum through the shared functions: no tree and no wave loop of their own
    for text in (step, fleet[fleet.index("void k_fleet_step"):]):
        assert "hull_chunk_partial(acc, res, part + 2 * c)" in text and "hull_body_sum(part, 0, " in text
        assert "red[" not in text and "off >>= 1" not in text
    # the order of the sum is written once: the shuffle tree stands in hull_wave_sum and nowhere else
    wave = hull[hull.index("void hull_wave_sum("):hull.index("void hull_chunk_partial(")]
    assert hull.count("__shfl_down") == wave.count("__shfl_down") == 2
    assert "__shfl_down" not in src and "__shfl_down" not in fleet
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "__threadfence" not in code and "volatile" not in code
