"""CPU tier of the footprint surface query at mesh edges (csrc/surface_query.h through tests/surface_query_shim.cpp, strict float32).

The families of tests/surface_edges.py -- vertex exactness and grid lines in rest mode at unit widths that are no power of two, world-mode
points ON vertices, edges and diagonals, 2 x 2 and 3 x 3 meshes, points off the displaced footprint, every iteration count, a broken vertex
-- on the g++ build, which keeps the float64 references honest before tests/test_surface_query_edges_gpu.py holds the device kernels to
them through mw_debug_query_mesh; and that hook's malformed calls, which need no GPU."""
import ctypes as C

import numpy as np
import pytest

import surface_edges as E
import surface_ref as S
from test_surface_query_cpu import build_shim, query


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(str(tmp_path_factory.mktemp("sqe") / "libsq_shim.so"))


@pytest.fixture(scope="module")
def q(shim):
    return lambda M, mode, xz, iters=0: query(shim, M.R, M.uw, M.vert, M.norm, M.white, 1, 0 if mode == "rest" else 1, xz, iters)


def test_windowed_reference_is_the_brute_force():
    """S.world_reference / S.on_mesh_rows look only at the triangles a point can lie on; on a sample they name what containing() names
    among all triangles."""
    R, uw, fold = 33, 1.0, 0.9
    M = E.mesh(R, uw, fold)
    xz = E.feature_points(R, uw, fold)[::7]
    count, local, ref, _ = S.world_reference(xz, np.zeros(len(xz)), M.vert, M.norm, M.white, R, uw, 1e-6)
    hits = S.world_hits(xz, M.vert, S.grid_triangles(R), 1e-6)
    assert np.array_equal(count, [len(t) for t, _ in hits]) and local[count > 0].all()   # (33 cells: the window is inside the mesh, no repeats)
    k = int(np.nonzero(count == 1)[0][0])
    t, w = hits[k]
    p, n, wh = S._interp(S.grid_triangles(R)[t[0]], w[0], M.vert, M.norm, M.white)
    np.testing.assert_allclose(ref[k], np.concatenate([p, n, [wh]]), rtol=1e-12, atol=1e-12)
    res = np.concatenate([ref[count > 0][:50, :3], ref[count > 0][:50, :3] + [0.0, 1.0, 0.0]])
    got = S.on_mesh_rows(res, M.vert, R, uw, 1e-4, 1e-4 * M.scale + 1e-6)
    want = [S.on_mesh(r, M.vert, S.grid_triangles(R), 1e-4, 1e-4 * M.scale + 1e-6) for r in res]
    assert np.array_equal(got, want) and got[:50].all() and not got[50:].any()


@pytest.mark.parametrize("R,uw", E.REST_CASES)
def test_rest_mode_vertices_exactly_and_grid_lines(q, R, uw):
    M = E.mesh(R, uw, 0.9)
    E.rest_vertices(q, M)
    E.rest_grid_lines(q, M)


@pytest.mark.parametrize("R,uw,fold", E.UNFOLDED)
@pytest.mark.parametrize("iters", [0, 16])
def test_world_mode_on_vertices_edges_and_diagonals(q, R, uw, fold, iters):
    dy, dr, noff = E.world_features(q, E.mesh(R, uw, fold), iters)
    print(f"R={R} uw={uw} fold={fold} iterations={iters}: largest height error {dy:.2e} of scale, largest residual {dr:.2e} uw, "
          f"{noff} border midpoints off the footprint")


@pytest.mark.parametrize("R", [2, 3])
@pytest.mark.parametrize("uw", [0.7, 2.5])
def test_world_mode_on_tiny_meshes(q, R, uw):
    E.world_tiny(q, E.mesh(R, uw, 0.6))


@pytest.mark.parametrize("R,uw,fold", E.UNFOLDED)
def test_world_points_off_the_footprint(q, R, uw, fold):
    M = E.mesh(R, uw, fold)
    for dist in E.RING_DISTS:
        _, excess = E.off_footprint(q, M, E.ring(R, uw, fold, dist))
        print(f"R={R} uw={uw} fold={fold} dist={dist}: largest (residual - border distance) / uw = {excess:.4f}")


def test_iterations_never_lose_ground_and_zero_means_eight(q):
    E.iterations(q)


@pytest.mark.parametrize("kind", E.DEFECTS)
@pytest.mark.parametrize("iters", [0, 64])
def test_a_defective_vertex_spoils_nothing_away_from_it(q, kind, iters):
    nfar, ndiff = E.defects(q, kind, iters)
    print(f"{kind} iterations={iters}: {nfar} rows held to the clean mesh's bits, {ndiff} rows differ")
    assert nfar > (10000 if iters == 0 else -1)


def test_hook_is_exported_and_refuses_malformed_calls_without_a_gpu(mw):
    """mw_debug_query_mesh: a hook, not part of the boundary; every malformed call is MW_EINVAL before the device is touched."""
    from mistral_water import _native
    L = C.CDLL(_native.LIB_PATH)
    assert hasattr(L, "mw_debug_query_mesh")
    assert "mw_debug_query_mesh" in _native.HOOK_SYMBOLS and "mw_debug_query_mesh" not in _native.ABI_SYMBOLS
    R = 4
    vert, norm, white, vel = (np.zeros((R * R, k), np.float32) for k in (3, 3, 1, 3))
    xz, out, vout = np.zeros((5, 2), np.float32), np.full((5, 8), 7.0, np.float32), np.full((5, 4), 7.0, np.float32)
    p = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)

    def st(R=R, uw=1.0, vert=vert, norm=norm, white=white, wstride=1, vel=None, mode=1, iters=0, xz=xz, n=5, out=out, vout=None):
        return mw.lib().mw_debug_query_mesh(R, uw, p(vert), p(norm), p(white), wstride, p(vel), mode, iters, p(xz), n, p(out), p(vout))
    for bad in (dict(R=1), dict(R=0), dict(uw=0.0), dict(uw=-1.0), dict(uw=float("nan")), dict(iters=-1), dict(iters=65), dict(n=-1),
                dict(mode=2), dict(wstride=2), dict(xz=None), dict(out=None), dict(vert=None), dict(norm=None), dict(white=None),
                dict(vel=vel, vout=None), dict(n=2 ** 32)):
        assert st(**bad) == mw.MW_EINVAL, bad
        assert b"mw_debug_query_mesh" in mw.lib().mw_last_error()
    assert st(n=0, xz=None, out=None, vert=None, norm=None, white=None) == mw.MW_OK     # an empty call reads no array
    assert (out == 7.0).all() and (vout == 7.0).all()
