"""CPU tier of the mixed fleets (mw_ocean_fleet_forces / mw_ocean_step_fleet and their device forms, include/mistral_water.h).

* the work mapping of csrc/fleet.h (fleet_table, fleet_map) through tests/fleet_shim.cpp (g++, strict float32): for hand-made hull
  tables every work index of the vertex, chunk and body spaces maps to the (hull, body, item) a plain Python enumeration gives;
* the wrench step (fleet_integrate) against body_ref.step fed F + Fw and tau + tw formed in float32, and bit for bit against
  body_integrate with no wrench; the wrench-row check;
* pack_fleet and the layout of the coefficient rows; the four entry points and two constants are exported, declared and bound, and refuse a NULL handle without a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import body_ref as B
import hull_ref as H
import shim_build
from conftest import REPO

SHIM = os.path.join(REPO, "tests", "fleet_shim.cpp")
HDR = os.path.join(REPO, "mistral-water_amd", "csrc", "fleet.h")
ENTRY_POINTS = ("mw_ocean_fleet_forces", "mw_ocean_fleet_forces_device", "mw_ocean_step_fleet", "mw_ocean_step_fleet_device")
VERTS, CHUNKS, BODIES = 0, 1, 2


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def fs(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("fleet") / "libfleet_shim.so")
    L = shim_build.strict_f32(SHIM, path)
    L.fs_totals.restype = None
    L.fs_totals.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
    L.fs_map_all.restype = None
    L.fs_map_all.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_int, C.c_void_p]
    L.fs_integrate.restype = None
    L.fs_integrate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p]
    L.fs_body_integrate.restype = None
    L.fs_body_integrate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p]
    L.fs_wrench_valid.restype = None
    L.fs_wrench_valid.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return L


def _table(rows):
    """hull rows (nverts, ntris, nbodies) -> [n, 5] int32 with the ranges laid out one after the other"""
    out, v0, t0 = [], 0, 0
    for nv, nt, nb in rows:
        out.append((v0, nv, t0, nt, nb))
        v0, t0 = v0 + nv, t0 + nt
    return np.asarray(out, np.int32)


def _enumerate(table, take, space):
    """the plain enumeration: hull after hull, body after body, item after item -> rows (hull, body, item, body index in the call)"""
    out, first = [], 0
    for h, (_, nv, _, nt, nb) in enumerate(table):
        per = nv if space == VERTS else (max(nv, nt) + 255) // 256 if space == CHUNKS else 1
        if (take >> h) & 1:
            out += [(h, b, i, first + b) for b in range(nb) for i in range(per)]
        first += nb
    return np.asarray(out, np.int32).reshape(-1, 4)


_rng = np.random.default_rng(2)
TABLES = {
    "one_hull": [(300, 10, 7)],
    "two_hulls": [(8, 12, 3), (162, 320, 2)],
    "five_hulls_empty_first_middle_last": [(4, 4, 0), (255, 255, 2), (9, 5, 0), (256, 256, 3), (257, 257, 0)],
    "chunk_edges": [(255, 256, 2), (256, 257, 1), (257, 255, 2), (3, 257, 3), (600, 10, 2)],
    "thirty_two_hulls": [(int(_rng.integers(3, 40)), int(_rng.integers(1, 600)), int(_rng.integers(0, 4))) for _ in range(32)],
    "all_empty_but_last": [(5, 5, 0), (6, 6, 0), (7, 300, 4)],
}


@pytest.mark.parametrize("name", list(TABLES))
def test_work_mapping_matches_plain_enumeration(fs, name):
    table = _table(TABLES[name])
    n = len(table)
    full = (1 << n) - 1
    takes = [full, full & 0x55555555, full & 0xAAAAAAAA] if n > 1 else [full]
    for take in takes:
        totals = np.zeros(3, np.int32)
        fs.fs_totals(_p(table), n, take, _p(totals))
        for space in (VERTS, CHUNKS, BODIES):
            want = _enumerate(table, take, space)
            assert totals[space] == len(want), (take, space)
            got = np.full((len(want), 4), -1, np.int32)
            fs.fs_map_all(_p(table), n, take, space, _p(got))
            assert np.array_equal(got, want), (take, space, np.nonzero((got != want).any(1))[0][:5])
    # the chunk count is hull_chunks': decided by the vertices where there are more of them than triangles
    if name == "one_hull":
        assert totals[CHUNKS] == 7 * 2


def _random_spd(rng, n):
    out = []
    for _ in range(n):
        A = rng.standard_normal((3, 3))
        out.append(A @ A.T + 0.5 * np.eye(3))
    return np.array(out)


def _random_state(mw, rng, n):
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
    wrench = np.zeros((n, 8), np.float32)
    wrench[:, 0:3] = rng.standard_normal((n, 3)) * masses[:, None] * 5
    wrench[:, 4:7] = rng.standard_normal((n, 3)) * masses[:, None] * 2
    wrench[:, [3, 7]] = rng.standard_normal((n, 2))  # the spare floats of a wrench row are not read
    return bodies, mass, rows, wrench


def test_wrench_step_against_reference(mw, fs):
    """fleet_integrate = body_ref.step fed F + Fw and tau + tw formed in float32, to the bound of the integration test of
    tests/test_bodies_cpu.py (4e-6 of 1 + the largest entry, per group of the state)"""
    rng = np.random.default_rng(21)
    n = 400
    bodies, mass, rows, wrench = _random_state(mw, rng, n)
    rows[7] = np.nan  # a NaN row: the body stays, wrench or not
    g, h = 9.81, 1.0 / 120
    out = bodies.copy()
    ok = np.zeros(n, np.int32)
    fs.fs_integrate(_p(out), _p(rows), _p(mass), _p(wrench), n, g, h, _p(ok))
    assert ok[7] == 0 and np.array_equal(out[7].view(np.uint32), bodies[7].view(np.uint32))
    summed = rows.copy()
    summed[:, 0:3] = rows[:, 0:3] + wrench[:, 0:3]  # float32 adds
    summed[:, 4:7] = rows[:, 4:7] + wrench[:, 4:7]
    assert summed.dtype == np.float32
    for b in range(n):
        if b == 7:
            continue
        assert ok[b] == 1
        ref = B.step(bodies[b], summed[b], mass[b].astype(np.float64), g, h)
        assert np.array_equal(out[b, [3, 11, 15]], bodies[b, [3, 11, 15]])
        for sl in (slice(0, 3), slice(4, 8), slice(8, 11), slice(12, 15)):
            scale = 1.0 + np.abs(ref[sl]).max()
            assert np.abs(out[b, sl] - ref[sl]).max() <= 4e-6 * scale, (b, sl, out[b, sl], ref[sl])
    # the same thing said with bits: the wrench step is body_integrate on the float32 sums
    direct = bodies.copy()
    fs.fs_body_integrate(_p(direct), _p(summed), _p(mass), n, g, h, _p(ok))
    assert np.array_equal(direct.view(np.uint32), out.view(np.uint32))
    assert not np.array_equal(direct[:7], bodies[:7])


def test_no_wrench_is_body_integrate_bit_for_bit(mw, fs):
    rng = np.random.default_rng(22)
    n = 300
    bodies, mass, rows, _ = _random_state(mw, rng, n)
    rows[11, 5] = np.nan
    a, b = bodies.copy(), bodies.copy()
    oka, okb = np.zeros(n, np.int32), np.zeros(n, np.int32)
    fs.fs_integrate(_p(a), _p(rows), _p(mass), None, n, 9.81, 0.01, _p(oka))
    fs.fs_body_integrate(_p(b), _p(rows), _p(mass), n, 9.81, 0.01, _p(okb))
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(oka, okb) and oka[11] == 0 and oka.sum() == n - 1


def test_wrench_row_check(fs):
    good = [1.0, -2.0, 3.0, 0.0, 0.5, 0.0, -0.25, 0.0]
    rows = np.array([good, [0.0] * 8,
                     [1.0, 2.0, 3.0, np.nan, 4.0, 5.0, 6.0, np.inf],  # the spare floats are not read
                     [np.nan] + good[1:], [1.0, np.inf] + good[2:], good[:2] + [-np.inf] + good[3:],
                     good[:4] + [np.nan] + good[5:], good[:5] + [np.inf] + good[6:], good[:6] + [np.nan, 0.0]], np.float32)
    ok = np.zeros(len(rows), np.int32)
    fs.fs_wrench_valid(_p(rows), len(rows), _p(ok))
    assert list(ok) == [1, 1, 1] + [0] * 6


def test_pack_fleet(mw):
    box, ico = H.box(1.0, 2.0, 3.0), H.icosphere(1.0, 1)
    x, t, table = mw.pack_fleet([(box[0], box[1], 3), (ico[0], ico[1], 0), (box[0], box[1], 5)])
    assert x.dtype == np.float32 and t.dtype == np.int32 and table.dtype == np.int32
    assert x.shape == (8 + 42 + 8, 3) and t.shape == (12 + 80 + 12, 3) and table.shape == (3, mw.MW_FLEET_NHULL)
    assert table.tolist() == [[0, 8, 0, 12, 3], [8, 42, 12, 80, 0], [50, 8, 92, 12, 5]]
    assert np.array_equal(t[12:92], ico[1]) and np.array_equal(x[8:50], ico[0])  # indices stay local to their hull
    with pytest.raises(ValueError):
        mw.pack_fleet([])


def test_fleet_coefficient_rows_are_laid_out_hull_by_hull(mw):
    """Ocean._fleet_coeffs hands the library [nhulls][5] rows in C order: one row broadcast to every hull, rows of their own, a NaN
    velocity scale replaced by the default, None"""
    o = mw.Ocean.__new__(mw.Ocean)  # no handle: the helper reads the parameters only
    o.semantics, o.params = mw.MW_SEM_FFTMESH, mw.MwParams(t_division=4.0)
    one = o._fleet_coeffs(3, [1000.0, 9.81, 20.0, 50.0, np.nan])
    assert one.dtype == np.float32 and one.shape == (3, 5) and one.flags["C_CONTIGUOUS"]
    assert np.array_equal(one.ravel(), np.float32([1000.0, 9.81, 20.0, 50.0, 0.25] * 3))
    own = o._fleet_coeffs(2, [[900.0, 9.0, 0.0, 0.0, 2.0], [1100.0, 10.0, 1.0, 2.0, np.nan]])
    assert own.flags["C_CONTIGUOUS"] and np.array_equal(own.ravel(), np.float32([900.0, 9.0, 0, 0, 2.0, 1100.0, 10.0, 1.0, 2.0, 0.25]))
    none = o._fleet_coeffs(2, None)
    assert none.flags["C_CONTIGUOUS"] and np.array_equal(none.ravel(), np.float32([1000.0, 9.81, 0, 0, 0.25] * 2))


def test_entry_points_exported_and_bound(mw):
    from mistral_water import _native
    L = mw.lib()
    hdr = open(os.path.join(REPO, "include", "mistral_water.h")).read()
    cs = open(os.path.join(REPO, "bindings", "csharp", "MistralWaterNative.cs")).read()
    for s in ENTRY_POINTS:
        assert hasattr(L, s) and s in _native.ABI_SYMBOLS and s + "(" in hdr and s + "(" in cs
    assert int(re.search(r"#define\s+MW_FLEET_MAX_HULLS\s+(\d+)", hdr).group(1)) == _native.MW_FLEET_MAX_HULLS == mw.MW_FLEET_MAX_HULLS == 32
    assert int(re.search(r"#define\s+MW_FLEET_NHULL\s+(\d+)", hdr).group(1)) == _native.MW_FLEET_NHULL == mw.MW_FLEET_NHULL == 5
    assert int(re.search(r"FleetMaxHulls\s*=\s*(\d+)", cs).group(1)) == 32 and int(re.search(r"FleetNHull\s*=\s*(\d+)", cs).group(1)) == 5
    assert int(re.search(r"#define\s+MW_FLEET_HULLS\s+(\d+)", open(HDR).read()).group(1)) == 32
    for name in ("fleet_forces", "fleet_forces_device", "step_fleet", "step_fleet_device"):
        assert callable(getattr(mw.Ocean, name))
    assert mw.lib().mw_abi_version() == 4


def test_null_handle_is_einval_without_a_gpu(mw):
    L = mw.lib()
    x, t, table = mw.pack_fleet([H.box(1.0, 1.0, 1.0) + (1,)])
    bodies = mw.pack_bodies([[0.0, 0.0, 0.0]])
    mass = mw.pack_mass(500.0, B.box_inertia(500.0, 1, 1, 1))
    cf = np.array([[1000.0, 9.81, 0, 0, 1]], np.float32)
    out = np.full((1, 8), 7.0, np.float32)
    before = bodies.copy()
    for fn in (L.mw_ocean_fleet_forces, L.mw_ocean_fleet_forces_device):
        assert fn(None, -1, _p(x), 8, _p(t), 12, _p(table), 1, _p(bodies), 1, _p(cf), 0, _p(out)) == mw.MW_EINVAL
        assert b"NULL handle" in L.mw_last_error()
    for fn in (L.mw_ocean_step_fleet, L.mw_ocean_step_fleet_device):
        assert fn(None, -1, _p(x), 8, _p(t), 12, _p(table), 1, _p(bodies), _p(mass), None, 1, _p(cf), C.c_float(0.1), 1, 0,
                  _p(out)) == mw.MW_EINVAL
        assert b"NULL handle" in L.mw_last_error()
    assert np.array_equal(bodies, before) and (out == 7.0).all()
