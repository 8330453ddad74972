"""CPU tier of the hull forces (mw_ocean_hull_forces / _device, include/mistral_water.h).

The MW_HD functions of csrc/hull_forces.h run on host arrays through tests/hull_forces_shim.cpp (g++, strict float32) and are checked
against tests/hull_ref.py (numpy float64):
* Archimedes on flat water: a closed hull gets (0, rho g V_submerged, 0) through the centre of buoyancy -- an axis-aligned box against
  the analytic volume, rotated boxes and an icosphere against the clipped-volume reference; fully submerged rho g V, fully dry zeros;
* on a wavy synthetic mesh (below and near the fold limit) the vertex step reads the water exactly where the surface and velocity
  queries read it, and the triangle step matches the reference, with vertices exactly at d = 0, degenerate triangles and NaN poses;
* the drag terms in isolation (rho = 0), linearity in the coefficients, and the exported entry points without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import hull_ref as H
import shim_build
import surface_ref as S
from conftest import REPO, has_gpu
from test_surface_query_cpu import build_shim as build_sq_shim, query as sq_query

SHIM = os.path.join(REPO, "tests", "hull_forces_shim.cpp")
VSHIM = os.path.join(REPO, "tests", "velocity_query_shim.cpp")
HDR = os.path.join(REPO, "mistral-water_amd", "csrc", "hull_forces.h")
RHO, G = 1000.0, 9.81
EPS = 2.0 ** -24


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def hs(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("hull") / "libhull_shim.so")
    L = shim_build.strict_f32(SHIM, path)
    L.hs_vertices.restype = C.c_int
    L.hs_vertices.argtypes = [C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_float, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                              C.c_void_p]
    for f in (L.hs_triangles, L.hs_rows):
        f.restype = None
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float,
                      C.c_void_p]
    L.hs_clip.restype = C.c_int
    L.hs_clip.argtypes = [C.c_void_p, C.c_void_p]
    return L


@pytest.fixture(scope="module")
def sqshim(tmp_path_factory):
    return build_sq_shim(str(tmp_path_factory.mktemp("sqh") / "libsq_shim.so"))


@pytest.fixture(scope="module")
def vshim(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("vqh") / "libvq_shim.so")
    L = shim_build.strict_f32(VSHIM, path)
    L.vq_shim_query.restype = C.c_int
    L.vq_shim_query.argtypes = [C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int, C.c_void_p]
    return L


class Water:
    """a synthetic displaced mesh the shim reads: vert [R*R, 3], vel [R*R, 3] or None"""

    def __init__(self, R, uw, vert, vel=None):
        self.R, self.uw = R, uw
        self.vert = np.ascontiguousarray(vert, np.float32)
        self.vel = None if vel is None else np.ascontiguousarray(vel, np.float32)


def flat_water(R=64, uw=1.0, level=0.0):
    rest = S.rest_plane(R, uw)
    return Water(R, uw, np.stack([rest[:, 0], np.full(R * R, level, np.float32), rest[:, 1]], 1))


def slab_of(hs, water, hull, tris, bodies, vscale=1.0, iters=0, drag=False):
    hull = np.ascontiguousarray(hull, np.float32)
    bodies = np.ascontiguousarray(bodies, np.float32).reshape(-1, 16)
    slab = np.empty((len(bodies), len(hull), 8), np.float32)
    vel = water.vel if drag else None
    assert hs.hs_vertices(water.R, water.uw, _p(water.vert), None if vel is None else _p(vel), vscale, iters, _p(hull), len(hull),
                          _p(bodies), len(bodies), _p(slab)) == 0
    return slab


def terms_of(hs, slab, tris, bodies, rho=RHO, g=G, lin=0.0, quad=0.0):
    tris = np.ascontiguousarray(tris, np.int32)
    bodies = np.ascontiguousarray(bodies, np.float32).reshape(-1, 16)
    out = np.empty((len(bodies), len(tris), 8), np.float32)
    hs.hs_triangles(_p(tris), len(tris), slab.shape[1], _p(np.ascontiguousarray(slab)), _p(bodies), len(bodies), rho, g, lin, quad, _p(out))
    return out


def rows_of(hs, slab, tris, bodies, rho=RHO, g=G, lin=0.0, quad=0.0):
    tris = np.ascontiguousarray(tris, np.int32)
    bodies = np.ascontiguousarray(bodies, np.float32).reshape(-1, 16)
    out = np.empty((len(bodies), 8), np.float32)
    hs.hs_rows(_p(tris), len(tris), slab.shape[1], _p(np.ascontiguousarray(slab)), _p(bodies), len(bodies), rho, g, lin, quad, _p(out))
    return out


def pack(p, q=None, v=None, w=None):
    import mistral_water
    return mistral_water.pack_bodies(p, q, v, w)


def _check_archimedes(terms, x64, tris, body, rho=RHO, g=G, vref=None):
    """summed terms against (0, rho g V, 0) and (r_B - p) x F; bound: 64 ulp of sum |contributions|"""
    F, tau = terms[:, 0:3].astype(np.float64).sum(0), terms[:, 4:7].astype(np.float64).sum(0)
    V, cB = H.submerged(x64, tris)
    if vref is not None:
        assert abs(V - vref) <= 1e-5 * vref, (V, vref)
    Fref = np.array([0.0, rho * g * V, 0.0])
    tref = np.cross(cB - np.asarray(body[0:3], np.float64), Fref)
    sF = np.abs(terms[:, 0:3].astype(np.float64)).sum() + 1e-30
    sT = np.abs(terms[:, 4:7].astype(np.float64)).sum() + 1e-30
    # the f32 vertices move the volume by up to ~ulp(coordinate) * area, far below the bound below for these unit-size hulls
    assert np.abs(F - Fref).max() <= 64 * EPS * sF + 1e-6 * rho * g * max(V, 1e-3), (F, Fref, sF)
    assert np.abs(tau - tref).max() <= 64 * EPS * sT + 1e-6 * rho * g * max(V, 1e-3), (tau, tref, sT)
    return F, tau


# ---- Archimedes on flat water --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("draft", [0.25, 0.5, 0.8125])
def test_archimedes_axis_aligned_box(hs, draft):
    """box 2 x 1 x 4 (w h l) floating at `draft`: V = w l draft, centre of buoyancy at half the draft below the water"""
    hull, tris = H.box(2.0, 1.0, 4.0)
    body = pack([[0.375, 0.5 - draft, -1.25]])
    slab = slab_of(hs, flat_water(), hull, tris, body)
    assert np.array_equal(slab[0, :, 3], (0 - slab[0, :, 1]).astype(np.float32))  # eta = 0 exactly
    terms = terms_of(hs, slab, tris, body)[0]
    F, tau = _check_archimedes(terms, H.transform(body, hull)[0], tris, body[0], vref=2.0 * 4.0 * draft)
    # centre of buoyancy (0.375, -draft/2, -1.25) vs the reference point: r_B - p = (0, -0.5, 0), parallel to F: no torque
    assert np.abs(tau).max() <= 64 * EPS * np.abs(terms[:, 4:7]).sum()
    wet = terms[:, 3].astype(np.float64).sum()
    assert abs(wet - (2 * 4 + 2 * (2 + 4) * draft)) <= 1e-5 * wet  # bottom + four walls up to the waterline


@pytest.mark.parametrize("seed", range(4))
def test_archimedes_rotated_boxes_and_icosphere(hs, seed):
    rng = np.random.default_rng(seed)
    for hull, tris in (H.box(2.0, 0.7, 3.0), H.icosphere(1.3)):
        q = H.random_quaternions(5, rng)
        p = np.stack([rng.uniform(-3, 3, 5), rng.uniform(-0.8, 0.8, 5), rng.uniform(-3, 3, 5)], 1).astype(np.float32)
        bodies = pack(p, q)
        slab = slab_of(hs, flat_water(), hull, tris, bodies)
        terms = terms_of(hs, slab, tris, bodies)
        x64 = H.transform(bodies, hull)
        for b in range(5):
            _check_archimedes(terms[b], x64[b], tris, bodies[b])


def test_fully_submerged_and_fully_dry(hs):
    hull, tris = H.icosphere(0.9)
    q = H.random_quaternions(2, np.random.default_rng(3))
    wet, dry = pack([[0.5, -2.0, 0.25]], q[:1]), pack([[0.5, 1.5, 0.25]], q[1:])
    w = flat_water()
    t = terms_of(hs, slab_of(hs, w, hull, tris, wet), tris, wet)[0]
    Vm = H.volume(H.transform(wet, hull)[0], tris)
    F = t[:, 0:3].astype(np.float64).sum(0)
    assert abs(F[1] - RHO * G * Vm) <= 64 * EPS * np.abs(t[:, 0:3]).sum() and np.abs(F[[0, 2]]).max() <= 64 * EPS * np.abs(t[:, 0:3]).sum()
    sd = slab_of(hs, w, hull, tris, dry)
    rows = rows_of(hs, sd, tris, dry, lin=3.0, quad=2.0)
    assert (rows[0, :7] == 0).all() and not np.signbit(rows[0, :7]).any() and rows[0, 7] == sd[0, :, 7].max()


# ---- the vertex step on waves ----------------------------------------------------------------------------------------------------
def _wavy(R, uw, fold, seed):
    vert, norm, white = S.synth_mesh(R, uw, fold, seed=seed)
    vel = np.random.default_rng(seed).standard_normal((R * R, 3)).astype(np.float32)
    return Water(R, uw, vert, vel), norm, white


def _bodies_over(water, n, rng, radius):
    rc = S.rest_coords(water.R, water.uw)
    dmax = float(np.abs(water.vert[:, [0, 2]] - S.rest_plane(water.R, water.uw)).max())
    lo, hi = float(rc[0]) + dmax + radius + water.uw, float(rc[-1]) - dmax - radius - water.uw
    p = np.stack([rng.uniform(lo, hi, n), rng.uniform(-0.5, 0.5, n), rng.uniform(lo, hi, n)], 1)
    return pack(p, H.random_quaternions(n, rng), rng.standard_normal((n, 3)), rng.standard_normal((n, 3)))


@pytest.mark.parametrize("R,uw,fold", [(48, 1.0, 0.5), (64, 0.5, 0.95)])
def test_vertex_step_reads_the_queries(hs, sqshim, vshim, R, uw, fold):
    """eta, residual and water velocity are those of the surface / velocity query shims at (x.x, x.z), bit for bit; x is the pose
    transform of the f64 reference to float32 rounding"""
    water, norm, white = _wavy(R, uw, fold, seed=R)
    rng = np.random.default_rng(R + 1)
    hull, tris = H.icosphere(1.1)
    bodies = _bodies_over(water, 6, rng, 1.1)
    for iters in (0, 16):
        slab = slab_of(hs, water, hull, tris, bodies, vscale=0.75, iters=iters, drag=True)
        x = slab[:, :, 0:3].reshape(-1, 3)
        ref = H.transform(bodies, hull).reshape(-1, 3)
        assert np.abs(x - ref).max() <= 4 * EPS * (np.abs(ref).max() + 2.0)
        xz = np.ascontiguousarray(x[:, [0, 2]])
        qs = sq_query(sqshim, R, uw, water.vert, norm, white, 1, 1, xz, iters)
        d = (qs[:, 1] - x[:, 1]).astype(np.float32)
        assert np.array_equal(slab[:, :, 3].reshape(-1).view(np.uint32), d.view(np.uint32))
        assert np.array_equal(slab[:, :, 7].reshape(-1).view(np.uint32), qs[:, 7].view(np.uint32))
        qv = np.empty((len(xz), 4), np.float32)
        assert vshim.vq_shim_query(R, uw, _p(water.vert), _p(water.vel), 1, _p(xz), len(xz), iters, _p(qv)) == 0
        assert np.array_equal(slab[:, :, 4:7].reshape(-1, 3), (qv[:, :3] * np.float32(0.75)).astype(np.float32))
    # drag off: no velocity is read
    slab = slab_of(hs, water, hull, tris, bodies, vscale=0.75, drag=False)
    assert (slab[:, :, 4:7] == 0).all()


# ---- the triangle step against the f64 reference --------------------------------------------------------------------------------
def _ref_rows(slab, tris, bodies, rho=RHO, g=G, lin=0.0, quad=0.0):
    return np.stack([H.forces(slab[b, :, 0:3], slab[b, :, 3], slab[b, :, 4:7], tris, bodies[b], rho, g, lin, quad)
                     for b in range(len(bodies))])


def _assert_rows(rows, terms, ref):
    """rows [n, 8] of the shim against the f64 reference [n, 7]; bound relative to sum |terms| per component group"""
    for b in range(len(ref)):
        for sl in (slice(0, 3), slice(3, 4), slice(4, 7)):
            scale = np.abs(terms[b, :, sl].astype(np.float64)).sum() + 1e-30
            err = np.abs(rows[b, sl].astype(np.float64) - ref[b, sl]).max()
            assert err <= 2e-5 * scale, (b, sl, err, scale)


@pytest.mark.parametrize("R,uw,fold", [(48, 1.0, 0.5), (64, 0.5, 0.95)])
def test_triangle_step_matches_reference_on_waves(hs, R, uw, fold):
    water, _, _ = _wavy(R, uw, fold, seed=R + 7)
    rng = np.random.default_rng(R)
    for hull, tris in (H.icosphere(1.2), H.box(1.5, 0.8, 2.5), H.grid_hull(4, 6, 2.0, 3.0, 0.6)):
        bodies = _bodies_over(water, 5, rng, 2.0)
        slab = slab_of(hs, water, hull, tris, bodies, vscale=1.0, drag=True)
        for lin, quad in ((0.0, 0.0), (35.0, 0.0), (0.0, 120.0), (20.0, 80.0)):
            terms = terms_of(hs, slab, tris, bodies, lin=lin, quad=quad)
            rows = rows_of(hs, slab, tris, bodies, lin=lin, quad=quad)
            assert np.isfinite(rows).all()
            _assert_rows(rows, terms, _ref_rows(slab, tris, bodies, lin=lin, quad=quad))
            # the rows are the terms summed
            assert np.allclose(rows[:, :7], terms[:, :, :7].astype(np.float64).sum(1), rtol=0, atol=1e-4 * np.abs(terms).sum(1).max())


def test_clip_cases(hs):
    """0, 1 and 2 sub-triangles, winding kept, cut points at d = 0 exactly, corners at d = 0 dry"""
    x = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1]], np.float32)
    u = np.arange(9, dtype=np.float32).reshape(3, 3)

    def run(d):
        inp = np.ascontiguousarray(np.concatenate([x, np.asarray(d, np.float32)[:, None], u], 1), np.float32)
        sub = np.zeros((2, 3, 7), np.float32)
        return hs.hs_clip(_p(inp), _p(sub)), sub

    def area(s):
        return 0.5 * np.cross(s[1, :3] - s[0, :3], s[2, :3] - s[0, :3])
    full = area(np.concatenate([x, np.zeros((3, 4))], 1))
    for d, n, frac in (([-1, -1, -1], 0, 0.0), ([0, 0, 0], 0, 0.0), ([1, 2, 3], 1, 1.0), ([1, -1, -1], 1, 0.25), ([1, -3, -3], 1, 1 / 16),
                       ([-1, 1, 1], 2, 0.75), ([0, 1, 1], 2, 1.0), ([1, 0, 0], 1, 1.0), ([1, 0, -1], 1, 0.5)):
        k, sub = run(d)
        assert k == n, d
        a = sum(area(sub[i]) for i in range(k)) if k else np.zeros(3)
        assert np.allclose(a, frac * full, atol=1e-7), (d, a, frac * full)
        for i in range(k):  # winding: every sub-triangle's area vector points the way of the triangle's (or is 0: a corner at d = 0)
            assert float(area(sub[i]) @ full) >= 0
            assert (sub[i, :, 3] >= 0).all()
        ref = H.clip(x.astype(np.float64), np.asarray(d, np.float64), u.astype(np.float64))
        assert len(ref) == k


def test_waterline_vertices_and_degenerate_triangles(hs):
    """vertices exactly at d = 0 (a box whose bottom or top sits on the water), degenerate triangles (repeated and collinear corners):
    no NaN, nothing counted twice, the reference's answer"""
    hull, tris = H.box(2.0, 1.0, 2.0)
    w = flat_water()
    on_bottom, on_top = pack([[0.5, 0.5, 0.5]]), pack([[0.5, -0.5, 0.5]])
    rows = rows_of(hs, slab_of(hs, w, hull, tris, on_bottom), tris, on_bottom)
    assert (rows[0, :7] == 0).all()  # the bottom face touches the water: no depth, no force
    sl = slab_of(hs, w, hull, tris, on_top)
    rows = rows_of(hs, sl, tris, on_top)
    assert abs(rows[0, 1] - RHO * G * 4.0) <= 1e-6 * RHO * G * 4.0 and np.abs(rows[0, [0, 2]]).max() <= 1e-3
    assert abs(rows[0, 3] - (4 + 4 * 2)) <= 1e-5 * 12  # bottom and walls; the top (d = 0) is not wet
    # extra degenerate triangles: repeated corners add exact zeros; a collinear one (a, midpoint of ab, b: collinear up to the float32
    # rounding of the transformed midpoint) adds at most rounding
    rng = np.random.default_rng(5)
    bodies = pack(rng.uniform(-1, 1, (6, 3)) * [1, 0.6, 1], H.random_quaternions(6, rng), rng.standard_normal((6, 3)))
    bodies[0, :3] = [0.5, -0.5, 0.5]
    bodies[0, 4:8] = [0, 0, 0, 1]
    rep = np.concatenate([tris, [[0, 0, 1], [2, 2, 2], [0, 1, 1]]]).astype(np.int32)
    mid = np.concatenate([hull, [(hull[0] + hull[1]) / 2]]).astype(np.float32)
    col = np.concatenate([rep, [[0, len(hull), 1]]]).astype(np.int32)
    sa = slab_of(hs, w, hull, tris, bodies)
    a = rows_of(hs, sa, tris, bodies, lin=5.0, quad=7.0)
    b = rows_of(hs, sa, rep, bodies, lin=5.0, quad=7.0)
    assert np.isfinite(b).all() and np.array_equal(a, b)
    slab = slab_of(hs, w, mid, col, bodies)
    c = rows_of(hs, slab, col, bodies, lin=5.0, quad=7.0)
    assert np.isfinite(c).all()
    _assert_rows(c, terms_of(hs, slab, col, bodies, lin=5.0, quad=7.0), _ref_rows(slab, col, bodies, lin=5.0, quad=7.0))
    assert np.abs(c[:, :7] - a[:, :7]).max() <= 1e-5 * np.abs(a[:, :7]).max()


def test_nan_pose_gives_a_nan_row(hs):
    hull, tris = H.icosphere()
    w = flat_water()
    bodies = pack([[0.0, 0.0, 0.0], [1.0, np.nan, 0.0], [1.0, 0.0, 2.0], [np.inf, 0.0, 0.0], [0.0, 0.0, 1.0]])
    bodies[4, 4:8] = [np.nan, 0, 0, 1]
    rows = rows_of(hs, slab_of(hs, w, hull, tris, bodies), tris, bodies, lin=1.0)
    assert np.isnan(rows[[1, 3, 4]]).all() and np.isfinite(rows[[0, 2]]).all()
    # a triangle index out of range: every row NaN, nothing read
    bad = tris.copy()
    bad[7, 1] = len(hull)
    rows = rows_of(hs, slab_of(hs, w, hull, tris, bodies[[0, 2]]), bad, bodies[[0, 2]])
    assert np.isnan(rows).all()


# ---- drag in isolation, linearity -----------------------------------------------------------------------------------------------
def test_linear_drag_in_still_water(hs):
    """rho = 0, still water, a translating body: F = -c A_wet v (f64 of the returned wetted area), torque sum (c_i - p) x F_i"""
    hull, tris = H.box(2.0, 1.0, 3.0)
    w = flat_water()
    w.vel = np.zeros_like(w.vert)
    rng = np.random.default_rng(11)
    bodies = pack(rng.uniform(-1, 1, (4, 3)) * [1, 0.4, 1], H.random_quaternions(4, rng), rng.standard_normal((4, 3)))
    slab = slab_of(hs, w, hull, tris, bodies, drag=True)
    rows = rows_of(hs, slab, tris, bodies, rho=0.0, lin=42.0)
    for b in range(4):
        ref = -42.0 * float(rows[b, 3]) * bodies[b, 8:11].astype(np.float64)
        assert np.abs(rows[b, 0:3] - ref).max() <= 1e-5 * np.abs(ref).max(), (rows[b], ref)
    _assert_rows(rows, terms_of(hs, slab, tris, bodies, rho=0.0, lin=42.0), _ref_rows(slab, tris, bodies, rho=0.0, lin=42.0))


def test_quadratic_drag_only_on_advancing_faces(hs):
    """a box 2 x 1 x 3 floating at draft 0.4 moving +x: only the +x wall (submerged area 3 x 0.4) advances, F = -q A v^2 x;
    moving straight up no face advances into the water: no quadratic drag at all"""
    hull, tris = H.box(2.0, 1.0, 3.0)
    w = flat_water()
    w.vel = np.zeros_like(w.vert)
    fwd = pack([[0.0, 0.1, 0.0]], None, [[1.5, 0.0, 0.0]])
    rows = rows_of(hs, slab_of(hs, w, hull, tris, fwd, drag=True), tris, fwd, rho=0.0, quad=50.0)
    ref = -50.0 * (3.0 * 0.4) * 1.5 ** 2
    assert abs(rows[0, 0] - ref) <= 1e-5 * abs(ref) and rows[0, 1] == 0 and rows[0, 2] == 0
    up = pack([[0.0, 0.1, 0.0]], None, [[0.0, 2.0, 0.0]])
    rows = rows_of(hs, slab_of(hs, w, hull, tris, up, drag=True), tris, up, rho=0.0, quad=50.0)
    assert (rows[0, :3] == 0).all()
    # the water moving against a still body is the same relative velocity
    w.vel[:, 0] = -1.5
    still = pack([[0.0, 0.1, 0.0]])
    rows2 = rows_of(hs, slab_of(hs, w, hull, tris, still, drag=True), tris, still, rho=0.0, quad=50.0)
    assert abs(rows2[0, 0] - ref) <= 1e-5 * abs(ref)


def test_forces_are_linear_in_the_coefficients(hs):
    water, _, _ = _wavy(48, 1.0, 0.6, seed=9)
    rng = np.random.default_rng(9)
    hull, tris = H.icosphere(1.0)
    bodies = _bodies_over(water, 4, rng, 1.0)
    slab = slab_of(hs, water, hull, tris, bodies, drag=True)
    base = rows_of(hs, slab, tris, bodies)
    # powers of two scale every float32 term exactly
    assert np.array_equal(rows_of(hs, slab, tris, bodies, rho=2 * RHO)[:, [0, 1, 2, 4, 5, 6]], 2 * base[:, [0, 1, 2, 4, 5, 6]])
    assert np.array_equal(rows_of(hs, slab, tris, bodies, g=4 * G)[:, [0, 1, 2, 4, 5, 6]], 4 * base[:, [0, 1, 2, 4, 5, 6]])
    lin = rows_of(hs, slab, tris, bodies, rho=0.0, lin=3.0)
    quad = rows_of(hs, slab, tris, bodies, rho=0.0, quad=5.0)
    assert np.array_equal(rows_of(hs, slab, tris, bodies, rho=0.0, lin=6.0)[:, :3], 2 * lin[:, :3])
    both = rows_of(hs, slab, tris, bodies, lin=3.0, quad=5.0)
    parts = base.astype(np.float64) + lin + quad
    for sl in (slice(0, 3), slice(4, 7)):
        sc = np.abs(base[:, sl]).max() + np.abs(lin[:, sl]).max() + np.abs(quad[:, sl]).max()
        assert np.abs(both[:, sl] - parts[:, sl]).max() <= 1e-5 * sc
    # any factor: linear to rounding
    r3 = rows_of(hs, slab, tris, bodies, rho=3 * RHO)
    assert np.allclose(r3[:, :3], 3 * base[:, :3].astype(np.float64), rtol=1e-5, atol=1e-5 * np.abs(base[:, :3]).max())


# ---- the ABI -------------------------------------------------------------------------------------------------------------------
def test_hull_symbols_exported_and_declared(mw):
    from mistral_water import _native
    L = C.CDLL(_native.LIB_PATH)
    hdr = open(_native.HEADER_PATH).read()
    for s in ("mw_ocean_hull_forces", "mw_ocean_hull_forces_device"):
        assert hasattr(L, s) and s in _native.ABI_SYMBOLS and s + "(" in hdr
    assert int(re.search(r"#define\s+MW_HULL_NCOEFFS\s+(\d+)", hdr).group(1)) == _native.MW_HULL_NCOEFFS == 5
    cs = open(os.path.join(REPO, "bindings", "csharp", "MistralWaterNative.cs")).read()
    assert int(re.search(r"HullNCoeffs\s*=\s*(\d+)", cs).group(1)) == 5


def test_hull_bad_arguments_are_statuses(mw):
    L = mw.lib()
    hull, tris = H.box(1, 1, 1)
    bodies = pack([[0, 0, 0]])
    cf = np.array([RHO, G, 0, 0, 1], np.float32)
    out = np.zeros((1, 8), np.float32)
    for fn in (L.mw_ocean_hull_forces, L.mw_ocean_hull_forces_device):
        assert fn(None, -1, _p(hull), len(hull), _p(tris), len(tris), _p(bodies), 1, _p(cf), 0, _p(out)) == mw.MW_EINVAL
        assert b"NULL handle" in L.mw_last_error()
    assert (out == 0).all()


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a GPU-less host")
def test_hull_without_gpu_is_an_error_status(mw):
    h = C.c_void_p()
    p = mw.MwParams()
    mw.lib().mw_params_default(C.byref(p), mw.MW_SEM_FFTMESH)
    assert mw.lib().mw_ocean_create(C.byref(p), C.byref(h)) == mw.MW_EDEVICE and not h.value
    hull, tris = H.box(1, 1, 1)
    out = np.full((1, 8), 7.0, np.float32)
    cf = np.array([RHO, G, 0, 0, 1], np.float32)
    assert mw.lib().mw_ocean_hull_forces(h, -1, _p(hull), 8, _p(tris), 12, _p(pack([[0, 0, 0]])), 1, _p(cf), 0, _p(out)) != mw.MW_OK
    assert (out == 7.0).all()


def test_hull_kernels_use_the_hd_functions():
    """the kernels' bodies are the functions the shim runs; no float atomics anywhere in the feature"""
    src = open(HDR).read()
    assert "hull_vertex(a.m, a.vel, a.vscale, a.iters, body, h, s)" in src[src.index("void k_hull_vertices"):]
    assert "hull_triangle(idx, a.nverts, vs, body, a.cf, acc)" in src[src.index("void k_hull_triangles"):]
    assert "hull_row(acc, res, o)" in src[src.index("void k_hull_reduce"):]
    assert "sq_locate(m, MW_SQ_WORLD, x[0], x[2], iters," in src
    assert "atomic" not in src.lower().replace("no atomics", "").replace("no float atomics", "")
