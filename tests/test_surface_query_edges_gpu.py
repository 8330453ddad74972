"""GPU tier of the footprint surface query at mesh and launch edges: the default (contracted) device build of k_query_surface<SqMesh> and
k_query_velocity<SqMesh>, which no shim gives the bits of.

Through mw_debug_query_mesh (the services' own launches on a caller's mesh): every family of tests/surface_edges.py with the assertions and
tolerances tests/test_surface_query_edges_cpu.py holds the strict g++ build to; the device against that build row by row; folded meshes;
the off-footprint excess against the shim's; the velocity kernel beside the surface kernel on every call; the whitecap stride.
Through real handles: frames with unit_width != 1 and odd R, and the device forms at batch sizes around the 256-lane block between guard
bands."""
import numpy as np
import pytest

import surface_edges as E
import surface_ref as S
import workloads
from test_surface_query_cpu import build_shim, query

pytestmark = pytest.mark.gpu

GUARD = 4096   # guard floats on each side of a device output, as tests/test_rigging_gpu.py


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class HookQuery:
    """q of tests/surface_edges.py on the device.  Every call runs the velocity kernel too, on the mesh's random per-vertex velocities, and
    holds its residual to the bits of the surface kernel's (both locate through sq_locate); the velocity rows stay in .vout."""

    def __init__(self, mw):
        self.mw, self.vout = mw, None

    def __call__(self, M, mode, xz, iters=0, wstride=1):
        out, self.vout = self.mw.Ocean.query_mesh(M.R, M.uw, M.vert, M.norm, M.white, xz, mode=mode, iterations=iters, vel=M.vel,
                                                   wstride=wstride)
        assert np.array_equal(_bits(self.vout[:, 3]), _bits(out[:, 7]))
        return out


@pytest.fixture(scope="module")
def q(mw):
    return HookQuery(mw)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return build_shim(str(tmp_path_factory.mktemp("sqe") / "libsq_shim.so"))


@pytest.fixture(scope="module")
def qs(shim):
    return lambda M, mode, xz, iters=0: query(shim, M.R, M.uw, M.vert, M.norm, M.white, 1, 0 if mode == "rest" else 1, xz, iters)


# ---- through the hook: the families of the CPU tier -------------------------------------------------------------------------------------
@pytest.mark.parametrize("R,uw", E.REST_CASES)
def test_rest_mode_vertices_exactly_and_grid_lines(q, R, uw):
    """The header's promise on the device's contracted build: a vertex's own rest position gives the vertex, its whitecap and (velocity
    kernel) its velocity exactly, at unit widths where (x - a) / (b - a) is not trivially exact."""
    M = E.mesh(R, uw, 0.9)
    E.rest_vertices(q, M)
    assert np.array_equal(q.vout[:, :3], M.vel) and (q.vout[:, 3] == 0).all()
    E.rest_grid_lines(q, M)


@pytest.mark.parametrize("R,uw,fold", E.UNFOLDED)
@pytest.mark.parametrize("iters", [0, 16])
def test_world_mode_on_vertices_edges_and_diagonals(q, R, uw, fold, iters):
    M = E.mesh(R, uw, fold)
    keep = {}

    def run(*a):
        keep["out"] = q(*a)
        return keep["out"]
    dy, dr, noff = E.world_features(run, M, iters, vel_of=lambda: q.vout)
    print(f"device R={R} uw={uw} fold={fold} iterations={iters}: largest height error {dy:.2e} of scale, largest residual {dr:.2e} uw, "
          f"{noff} border midpoints off the footprint")
    # check_world's bounds point by point on a sample (pure Python: 600 points)
    xz = E.feature_points(R, uw, fold)
    pick = np.sort(np.random.default_rng(R).choice(len(xz), min(600, len(xz)), replace=False))
    S.check_world(keep["out"][pick], xz[pick], M.vert, M.norm, M.white, uw, S.all_triangles(R), unique_exact=True)


@pytest.mark.parametrize("R", [2, 3])
@pytest.mark.parametrize("uw", [0.7, 2.5])
def test_world_mode_on_tiny_meshes(q, R, uw):
    E.world_tiny(q, E.mesh(R, uw, 0.6))


@pytest.mark.parametrize("R,uw,fold", E.UNFOLDED)
def test_world_points_off_the_footprint(q, qs, R, uw, fold):
    """... and the clamped walk's answer is no further from the border on the device than the strict build's on the same points (1e-4
    unit widths of slack: the two builds round differently)."""
    M = E.mesh(R, uw, fold)
    for dist in E.RING_DISTS:
        xz = E.ring(R, uw, fold, dist)
        _, dev = E.off_footprint(q, M, xz)
        _, cpu = E.off_footprint(qs, M, xz)
        print(f"R={R} uw={uw} fold={fold} dist={dist}: largest (residual - border distance) / uw = {dev:.4f} on the device, {cpu:.4f} in the shim")
        assert dev <= cpu + 1e-4, (dist, dev, cpu)


def test_iterations_never_lose_ground_and_zero_means_eight(q):
    E.iterations(q)


@pytest.mark.parametrize("kind", E.DEFECTS)
@pytest.mark.parametrize("iters", [0, 64])
def test_a_defective_vertex_spoils_nothing_away_from_it(q, kind, iters):
    nfar, ndiff = E.defects(q, kind, iters)
    print(f"device {kind} iterations={iters}: {nfar} rows held to the clean mesh's bits, {ndiff} rows differ")
    assert nfar > (10000 if iters == 0 else -1)


# ---- the device against the strict shim ---------------------------------------------------------------------------------------------------
SHIM_MESHES = [(17, 0.7, 0.5, 7), (33, 1.0, 0.9, 7), (64, 0.5, 0.95, 7), (64, 1.0, 0.99, 7), (32, 1.0, 2.5, 3), (64, 1.0, 3.0, 3)]
MAX_DIFFERING = 40   # of 20 000 rows (0.2 %): contraction may flip an in-triangle decision; g++'s contraction flips at most 5 on these inputs


@pytest.mark.parametrize("R,uw,fold,seed0", SHIM_MESHES)
@pytest.mark.parametrize("iters", [0, 24])
def test_device_rows_against_the_strict_shim(q, qs, R, uw, fold, seed0, iters):
    M = E.mesh(R, uw, fold, seed=seed0 + R)
    rc = S.rest_coords(R, uw)
    xz = np.random.default_rng(9).uniform(float(rc[0]) - 4 * uw, float(rc[-1]) + 4 * uw, (20000, 2)).astype(np.float32)
    dev, cpu = q(M, "world", xz, iters), qs(M, "world", xz, iters)
    assert np.isfinite(dev).all() and np.isfinite(cpu).all()
    dy = np.abs(dev[:, 1].astype(np.float64) - cpu[:, 1])
    dr = np.abs(dev[:, 7].astype(np.float64) - cpu[:, 7])
    dxz = np.abs(dev[:, [0, 2]].astype(np.float64) - cpu[:, [0, 2]]).max(1)
    differs = (dy > 1e-5 * M.scale) | (dr > 1e-4 * uw) | (dxz > 1e-4 * uw)
    print(f"R={R} uw={uw} fold={fold} iterations={iters}: {int(differs.sum())} of {len(xz)} rows differ, "
          f"{int((_bits(dev) != _bits(cpu)).any(1).sum())} differ in some bit; largest dy {dy.max():.3e} (agreeing rows {dy[~differs].max():.3e}), "
          f"largest dr {dr.max():.3e} (agreeing rows {dr[~differs].max():.3e})")
    assert differs.sum() <= MAX_DIFFERING, int(differs.sum())
    if differs.any():   # a row that took another decision is still an answer: on the mesh, with its honest residual
        E.assert_on_mesh_and_honest(dev[differs], xz[differs], M)


@pytest.mark.parametrize("R,fold", [(32, 2.5), (64, 3.0)])
def test_world_mode_in_folds_is_on_the_mesh_with_an_honest_residual(q, R, fold):
    """tests/test_surface_query_cpu.py's folded case, its points and its conditions, on the device"""
    uw = 1.0
    M = E.mesh(R, uw, fold, seed=3 + R)
    rc = S.rest_coords(R, uw)
    xz = np.random.default_rng(3).uniform(float(rc[0]) - 2, float(rc[-1]) + 2, (500, 2)).astype(np.float32)
    out = q(M, "world", xz, 24)
    nuniq, nfold, nmissed = S.check_world(out, xz, M.vert, M.norm, M.white, uw, S.all_triangles(R), unique_exact=False)
    print(f"device R={R} fold={fold}: {nuniq} unique points resolved, {nmissed} trapped by a fold, {nfold} in folds")
    assert nfold > 10 and nuniq > 200 and nmissed <= 0.1 * nuniq


def test_whitecap_stride_changes_no_bit(q):
    M = E.mesh(33, 1.0, 0.9)
    for mode, xz in (("world", E.feature_points(33, 1.0, 0.9)), ("world", E.ring(33, 1.0, 0.9, 3.0)), ("rest", S.grid_line_points(33, 1.0))):
        assert np.array_equal(_bits(q(M, mode, xz, 0, wstride=1)), _bits(q(M, mode, xz, 0, wstride=4)))
    assert M.white.max() > M.white.min()


# ---- through real handles ---------------------------------------------------------------------------------------------------------------
def _fft64(mw):
    p = workloads.fftmesh_params(64, choppiness=1.5)
    uw = float(np.float32(0.7))
    return mw.Ocean(resolution=64, unit_width=uw, length=uw * 64, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude, choppiness=1.5,
                    gravity=p.gravity, device=0), 64, 0.7


def _czt33(mw):
    N, uw, L = 33, 0.7, 25.0
    return mw.Ocean(resolution=N, unit_width=uw, length=L, wind=(14.45, 12.0), amplitude=1.5e-8 * (1024.0 / N) ** 2 * (L / N) ** 2,
                    choppiness=1.2, device=0), N, uw


def _renderer8(mw):
    return mw.Ocean(resolution=8, unit_width=2.5, length=27.155, wind=(14.45, 12.0), amplitude=0.41, choppiness=1.5, mult=1.5, seed=1,
                    semantics=mw.MW_SEM_OCEANRENDERER, device=0), 8, 2.5


@pytest.mark.parametrize("make", [_fft64, _czt33, _renderer8], ids=["fft64_uw0.7", "chirpz33_uw0.7", "renderer8_uw2.5"])
def test_frames_with_other_unit_widths_and_odd_sizes(mw, make):
    o, R, uw = make(mw)
    with o:
        if make is _renderer8:
            for dt in (0.016, 0.5, 0.033):
                o.generate_texture(dt)
            v, n, white = o.displace_mesh()
        else:
            assert (o.max_batch > 1) == (make is _fft64)     # the FFT path, and the chirp-z path
            v, n, c = o.evaluate(1.7)
            white = c[:, 0].copy()
        white = np.ascontiguousarray(white).reshape(-1)
        rest = S.rest_plane(R, uw)
        assert np.array_equal(rest, o.rest_mesh()[0][:, [0, 2]])
        out = o.query_surface(rest, mode="rest")
        bad = np.nonzero((out[:, :3] != v).any(1) | (out[:, 6] != white))[0]
        assert len(bad) == 0, (len(bad), bad[:5], out[bad[:5]], v[bad[:5]])
        assert (out[:, 7] == 0).all()
        vel = o.velocity()
        qv = o.query_velocity(rest, mode="rest")
        assert np.array_equal(_bits(qv[:, :3]), _bits(vel)) and (qv[:, 3] == 0).all()
        xz = S.displaced_feature_points(v, R)
        w = o.query_surface(xz, mode="world")
    assert np.isfinite(w).all()
    count, local, ref, _ = S.world_reference(xz, w[:, 1], v, n, white, R, uw, 1e-6)
    held = (count > 0) & local            # the frame does not fold there: the triangles that hold the point meet at it
    scale, wscale = float(np.abs(v[:, 1]).max()), max(1.0, float(np.abs(white).max()))
    print(f"R={R} uw={uw}: {int(held.sum())} of {len(xz)} feature points held to their triangle; largest height error "
          f"{np.abs(w[held, 1] - ref[held, 1]).max() / scale:.2e} of scale, largest residual {w[held, 7].max() / uw:.2e} uw")
    assert held.sum() >= 0.5 * len(xz)
    assert np.abs(w[held, 1] - ref[held, 1]).max() <= 1e-5 * scale
    assert w[held, 7].max() <= 1e-4 * uw
    assert np.abs(w[held, 3:6] - ref[held, 3:6]).max() <= 1e-4 and np.abs(w[held, 6] - ref[held, 6]).max() <= 1e-4 * wscale


@pytest.mark.parametrize("mode", ["world", "rest"])
def test_device_forms_at_the_block_edges_between_guard_bands(mw, mode):
    """n = 1, 255, 256, 257, 513 (the 256-lane block and the grid rule (n + 255) / 256): the device forms write their n rows and nothing
    else -- the output stands at a 16-byte-aligned offset inside a sentinel-filled tensor, 4096 guard floats on each side -- and row k has
    the bits of the same point queried inside one batch of 100 003."""
    import torch
    o, R, uw = _fft64(mw)
    big_n, start = 100003, 777
    rc = S.rest_coords(R, uw)
    xz = np.random.default_rng(12).uniform(float(rc[0]) - 2 * uw, float(rc[-1]) + 2 * uw, (big_n, 2)).astype(np.float32)
    with o:
        o.evaluate(1.7)
        big = {"surface": o.query_surface(xz, mode=mode, iterations=12), "velocity": o.query_velocity(xz, mode=mode, iterations=12)}
        for name, per, fn in (("surface", 8, o.query_surface_device), ("velocity", 4, o.query_velocity_device)):
            for n in (1, 255, 256, 257, 513):
                d_xz = torch.from_numpy(xz[start:start + n].copy()).cuda()
                buf = torch.full((2 * GUARD + per * n,), 7.0, dtype=torch.float32, device="cuda")
                view = buf[GUARD:GUARD + per * n]
                assert view.data_ptr() % 16 == 0
                torch.cuda.synchronize()
                fn(d_xz.data_ptr(), n, view.data_ptr(), mode=mode, iterations=12)
                o.synchronize()
                got = buf.cpu().numpy()
                assert (got[:GUARD] == 7.0).all() and (got[GUARD + per * n:] == 7.0).all(), (name, n)
                assert np.array_equal(_bits(got[GUARD:GUARD + per * n].reshape(n, per)), _bits(big[name][start:start + n])), (name, n)
