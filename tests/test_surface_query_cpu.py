"""CPU tier of the surface queries (mw_ocean_query_surface, include/mistral_water.h).

* the two entry points are exported and refuse bad arguments with a status, never a crash, and without a GPU;
* the MW_HD query functions of csrc/surface_query.h, compiled with g++ (tests/surface_query_shim.cpp, strict float32 as
  tests/emul_build.py builds the kernels' phase functions), against the numpy brute-force reference of tests/surface_ref.py on
  synthetic choppy meshes below and beyond the fold limit."""
import ctypes as C
import os

import numpy as np
import pytest

import shim_build
import surface_ref as S
from conftest import REPO, has_gpu

SHIM = os.path.join(REPO, "tests", "surface_query_shim.cpp")
HDR = os.path.join(REPO, "mistral-water_amd", "csrc", "surface_query.h")


def build_shim(path, defs=()):
    L = shim_build.strict_f32(SHIM, path, defs)
    L.sq_shim_query.restype = C.c_int
    L.sq_shim_query.argtypes = [C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int64,
                                C.c_int, C.c_void_p]
    L.sq_shim_rest_coord.restype = C.c_float
    L.sq_shim_rest_coord.argtypes = [C.c_int, C.c_float, C.c_int]
    return L


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(str(tmp_path_factory.mktemp("sq") / "libsq_shim.so"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def query(shim, R, uw, vert, norm, white, wstride, mode, xz, iters=0):
    xz = np.ascontiguousarray(xz, np.float32)
    out = np.empty((len(xz), 8), np.float32)
    wh = np.ascontiguousarray(np.repeat(white[:, None], wstride, 1), np.float32)
    assert shim.sq_shim_query(R, uw, _p(vert), _p(norm), _p(wh), wstride, mode, _p(xz), len(xz), iters, _p(out)) == 0
    return out


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_query_symbols_exported_and_declared(mw):
    from mistral_water import _native
    L = C.CDLL(_native.LIB_PATH)
    for s in ("mw_ocean_query_surface", "mw_ocean_query_surface_device"):
        assert hasattr(L, s) and s in _native.ABI_SYMBOLS
    hdr = open(_native.HEADER_PATH).read()
    assert "#define MW_QUERY_REST 0" in hdr and "#define MW_QUERY_WORLD 1" in hdr
    assert _native.MW_QUERY_REST == 0 and _native.MW_QUERY_WORLD == 1


def test_query_bad_arguments_are_statuses(mw):
    """No handle can exist without a GPU: every malformed call is refused by status (MW_EINVAL), never by a crash."""
    L = mw.lib()
    xz = np.zeros((4, 2), np.float32)
    out = np.zeros((4, 8), np.float32)
    for fn in (L.mw_ocean_query_surface, L.mw_ocean_query_surface_device):
        assert fn(None, -1, 1, _p(xz), 4, 0, _p(out)) == mw.MW_EINVAL
        assert fn(None, -1, 1, None, 0, 0, None) == mw.MW_EINVAL
        assert b"NULL handle" in L.mw_last_error()


@pytest.mark.skipif(has_gpu(), reason="only meaningful on a GPU-less host")
def test_query_without_gpu_is_an_error_status(mw):
    """Without a GPU no handle can be made (MW_EDEVICE), and both query entry points, given what a caller then holds (no handle)
    and well-formed arrays, return an error status and leave the output alone: no CPU fallback answers."""
    import mistral_water as M
    h = C.c_void_p()
    p = M.MwParams()
    M.lib().mw_params_default(C.byref(p), M.MW_SEM_FFTMESH)
    assert M.lib().mw_ocean_create(C.byref(p), C.byref(h)) == M.MW_EDEVICE and not h.value
    xz = np.zeros((3, 2), np.float32)
    for fn in (M.lib().mw_ocean_query_surface, M.lib().mw_ocean_query_surface_device):
        out = np.full((3, 8), 7.0, np.float32)
        for mode in (0, 1):
            assert fn(h, -1, mode, _p(xz), 3, 0, _p(out)) != M.MW_OK
        assert (out == 7.0).all()


def test_query_kernel_uses_the_hd_functions():
    """the kernel body is the shared MW_HD function (what the shim below checks is what the GPU runs)"""
    src = open(HDR).read()
    k = src[src.index("__global__"):]
    assert "sq_query_point(m, mode, q.x, q.y, iters, r)" in k and "const float2 q = xz[k]" in k


# ---- the MW_HD functions against the brute-force reference ----------------------------------------------------------------
def test_rest_coords_and_triangles_match_the_library(shim, emul):
    """surface_ref's rest coordinates and triangle split are those of the product's rest mesh (rest_mesh_element)."""
    for R, uw in ((16, 1.0), (13, 0.7), (64, 2.5)):
        v, _, _, idx = emul.rest_mesh(R, uw)
        rc = S.rest_coords(R, uw)
        assert np.array_equal(rc, [shim.sq_shim_rest_coord(R, uw, a) for a in range(R)])
        assert np.array_equal(v[:, [0, 2]], S.rest_plane(R, uw))
        assert sorted(map(tuple, idx.reshape(-1, 3))) == sorted(map(tuple, S.grid_triangles(R)))


@pytest.mark.parametrize("R,uw,fold", [(16, 1.0, 0.5), (64, 0.5, 0.95), (17, 2.0, 0.9)])
def test_rest_mode_matches_brute_force(shim, R, uw, fold):
    vert, norm, white = S.synth_mesh(R, uw, fold, seed=R)
    rng = np.random.default_rng(1)
    rc = S.rest_coords(R, uw)
    lo, hi = float(rc[0]), float(rc[-1])
    pts = rng.uniform(lo, hi, (600, 2)).astype(np.float32)
    verts_rest = S.rest_plane(R, uw)
    off = np.array([[lo - 0.01, 0.0], [0.0, hi + 1.0], [np.nan, 0.0], [np.inf, 0.0]], np.float32)
    xz = np.concatenate([pts, verts_rest, off])
    out = query(shim, R, uw, vert, norm, white, 4, 0, xz)
    n = len(pts)
    ref = S.rest_reference(xz[:n], vert, norm, white, R, uw, S.grid_triangles(R))
    scale = float(np.abs(vert).max())
    assert np.abs(out[:n, :3] - ref[:, :3]).max() <= 1e-5 * scale
    assert np.abs(out[:n, 3:6] - ref[:, 3:6]).max() <= 1e-5
    assert np.abs(out[:n, 6] - ref[:, 6]).max() <= 1e-5 * max(1.0, float(white.max()))
    assert (out[:n, 7] == 0).all()
    # a vertex's own rest position gives that vertex exactly
    nv = R * R
    assert np.array_equal(out[n:n + nv, :3], vert)
    np.testing.assert_allclose(out[n:n + nv, 3:6], norm, rtol=1e-6, atol=1e-7)
    assert np.array_equal(out[n:n + nv, 6], white)
    assert np.isnan(out[n + nv:]).all()


@pytest.mark.parametrize("R,uw,fold,iters", [(16, 1.0, 0.6, 0), (64, 0.5, 0.95, 0), (64, 1.0, 0.99, 32), (33, 1.5, 0.9, 16)])
def test_world_mode_below_the_fold_limit(shim, R, uw, fold, iters):
    vert, norm, white = S.synth_mesh(R, uw, fold, seed=7 + R)
    rng = np.random.default_rng(2)
    rc = S.rest_coords(R, uw)
    dmax = float(np.abs(vert[:, [0, 2]] - S.rest_plane(R, uw)).max())
    lo, hi = float(rc[0]) + dmax + uw, float(rc[-1]) - dmax - uw
    xz = rng.uniform(lo, hi, (500, 2)).astype(np.float32)
    out = query(shim, R, uw, vert, norm, white, 1, 1, xz, iters)
    nuniq, nfold, _ = S.check_world(out, xz, vert, norm, white, uw, S.all_triangles(R))
    assert nfold == 0 and nuniq >= 0.9 * len(xz)


@pytest.mark.parametrize("R,fold", [(32, 2.5), (64, 3.0)])
def test_world_mode_in_folds_is_on_the_mesh_with_an_honest_residual(shim, R, fold):
    uw = 1.0
    vert, norm, white = S.synth_mesh(R, uw, fold, seed=3 + R)
    rng = np.random.default_rng(3)
    rc = S.rest_coords(R, uw)
    xz = rng.uniform(float(rc[0]) - 2, float(rc[-1]) + 2, (500, 2)).astype(np.float32)  # some off the displaced footprint
    out = query(shim, R, uw, vert, norm, white, 1, 1, xz, 24)
    nuniq, nfold, nmissed = S.check_world(out, xz, vert, norm, white, uw, S.all_triangles(R), unique_exact=False)
    print(f"R={R} fold={fold}: {nuniq} unique points resolved, {nmissed} trapped by a fold, {nfold} in folds")
    assert nfold > 10 and nuniq > 200 and nmissed <= 0.1 * nuniq


def test_world_mode_rejects_non_finite_points_and_rest_points_equal_world_points_of_an_undisplaced_mesh(shim):
    R, uw = 16, 1.0
    vert, norm, white = S.synth_mesh(R, uw, 0.0, seed=1)   # fold 0: no horizontal displacement
    rng = np.random.default_rng(4)
    rc = S.rest_coords(R, uw)
    xz = rng.uniform(float(rc[0]), float(rc[-1]), (200, 2)).astype(np.float32)
    a = query(shim, R, uw, vert, norm, white, 1, 0, xz)
    b = query(shim, R, uw, vert, norm, white, 1, 1, xz)
    np.testing.assert_allclose(a[:, :7], b[:, :7], rtol=0, atol=1e-5)
    assert b[:, 7].max() <= 1e-5
    bad = query(shim, R, uw, vert, norm, white, 1, 1, np.array([[np.nan, 0], [0, np.inf]], np.float32))
    assert np.isnan(bad).all()


def test_preconditioned_walk_resolves_what_the_plain_iteration_leaves(tmp_path):
    """Why the walk's steps are preconditioned (csrc/surface_query.h): near the fold limit the plain fixed-point step u <- (x, z) - D(u)
    contracts only by the largest eigenvalue of dD/du (-> 1), so a bounded number of steps leaves points unresolved.  Same mesh, same
    points, three builds of the MW_HD walk: plain steps, preconditioned steps capped at 1 cell, the product's (capped at 4 cells)."""
    R, uw = 128, 1.0
    vert, norm, white = S.synth_mesh(R, uw, 0.99, seed=7 + R)
    rc = S.rest_coords(R, uw)
    dmax = float(np.abs(vert[:, [0, 2]] - S.rest_plane(R, uw)).max())
    xz = np.random.default_rng(2).uniform(float(rc[0]) + dmax + uw, float(rc[-1]) - dmax - uw, (4000, 2)).astype(np.float32)
    walks = {"plain": build_shim(str(tmp_path / "plain.so"), ["MW_SQ_PRECONDITION=0"]),
             "cap1": build_shim(str(tmp_path / "cap1.so"), ["MW_SQ_MAX_STEP=1.f"]),
             "product": build_shim(str(tmp_path / "product.so"))}
    miss = {}
    for name, L in walks.items():
        for iters in (4, 8, 16):
            out = query(L, R, uw, vert, norm, white, 1, 1, xz, iters)
            miss[(name, iters)] = float(np.mean(out[:, 7] > 1e-4 * uw))
    print("unresolved fraction (128^2, 0.99 of the fold limit):", {f"{k[0]}/{k[1]}": round(v, 4) for k, v in miss.items()})
    assert miss[("plain", 8)] > 0.03 and miss[("plain", 16)] > 0.01
    assert miss[("cap1", 4)] > 0.03                       # a 1-cell cap needs more steps than the default allows ...
    assert miss[("product", 4)] <= 0.001 and miss[("product", 8)] == 0.0   # ... the 4-cell cap resolves every point in 4
