"""The edge families of the footprint surface query, written once for both tiers: tests/test_surface_query_edges_cpu.py runs them on the
g++ shim of csrc/surface_query.h, tests/test_surface_query_edges_gpu.py on the device kernels (mw_debug_query_mesh) -- the same inputs,
the same assertions, the same tolerances.

A family takes `q(M, mode, xz, iters) -> out [n, 8]`, the backend under test, and a Mesh M.  Points and references come from
tests/surface_ref.py (numpy, float64)."""
import functools
import math

import numpy as np

import surface_ref as S

MAX_STEP = 4.0       # MW_SQ_MAX_STEP (csrc/surface_query.h)
DEFAULT_ITERS = 8    # MW_SQ_DEFAULT_ITERS: what iterations = 0 means (sq_iters)

UNFOLDED = [(17, 0.7, 0.5), (33, 1.0, 0.9), (64, 0.5, 0.95)]          # (R, unit_width, fold): the meshes of most families
REST_CASES = [(R, uw) for R in (2, 3, 17, 64) for uw in (0.7, 1.0, 2.5)]
RING_DISTS = (0.25, 3.0, 40.0, 1e4)
ITER_COUNTS = (1, 2, 3, 4, 6, 8, 12, 16, 24, 32, 64)
DEFECTS = ("nan", "inf_x", "collapsed")


class Mesh:
    def __init__(self, R, uw, fold, seed):
        self.R, self.uw, self.fold = R, uw, fold
        self.vert, self.norm, self.white = S.synth_mesh(R, uw, fold, seed=seed)
        self.vel = np.random.default_rng(seed + 1000).standard_normal((R * R, 3)).astype(np.float32)
        for a in (self.vert, self.norm, self.white, self.vel):
            a.setflags(write=False)   # shared between tests: left unchanged

    @property
    def scale(self):      # the height scale of check_world
        return float(np.abs(self.vert[:, 1]).max())

    @property
    def wscale(self):
        return max(1.0, float(np.abs(self.white).max()))


@functools.lru_cache(maxsize=None)
def mesh(R, uw, fold, seed=None):
    """S.synth_mesh(R, uw, fold, seed = 7 + R unless given), made once"""
    return Mesh(R, uw, fold, 7 + R if seed is None else seed)


def _honest(out, xz):
    """|residual - |p.xz - q|| within check_world's bound, per row"""
    bound = 2e-6 * np.maximum(1.0, np.abs(xz.astype(np.float64)).max(1))
    d = np.hypot(out[:, 0].astype(np.float64) - xz[:, 0], out[:, 2].astype(np.float64) - xz[:, 1])
    return np.abs(out[:, 7] - d) <= bound, bound


def assert_on_mesh_and_honest(out, xz, M, vert=None):
    """Every row finite, a point of the mesh (check_world's bounds) with its horizontal distance from the query as the residual."""
    vert = M.vert if vert is None else vert
    assert np.isfinite(out).all(), xz[~np.isfinite(out).all(1)][:5]
    ok, _ = _honest(out, xz)
    assert ok.all(), (xz[~ok][:5], out[~ok][:5])
    on = S.on_mesh_rows(out, vert, M.R, M.uw, 1e-4, 1e-4 * M.scale + 1e-6)
    assert on.all(), (xz[~on][:5], out[~on][:5])


# ---- rest mode -------------------------------------------------------------------------------------------------------------------
def rest_vertices(q, M):
    """A vertex's own rest position returns the vertex: position and whitecap exactly (values: the accumulation starts from +0)."""
    out = q(M, "rest", S.rest_plane(M.R, M.uw), 0)
    bad = np.nonzero((out[:, :3] != M.vert).any(1) | (out[:, 6] != M.white))[0]
    assert len(bad) == 0, (len(bad), bad[:5], out[bad[:5]], M.vert[bad[:5]])
    assert (out[:, 7] == 0).all()
    np.testing.assert_allclose(out[:, 3:6], M.norm, rtol=1e-6, atol=1e-7)


def rest_grid_lines(q, M):
    """On and one float32 either side of every rest grid line: NaN exactly off the footprint, the brute-force answer elsewhere."""
    R, uw = M.R, M.uw
    xz = S.grid_line_points(R, uw)
    rc = S.rest_coords(R, uw)
    outside = ((xz < rc[0]) | (xz > rc[-1])).any(1)
    assert outside.any() and (xz == rc[0]).any(1)[~outside].any() and (xz == rc[-1]).any(1)[~outside].any()
    ref = S.rest_reference(xz, M.vert, M.norm, M.white, R, uw, S.grid_triangles(R))
    assert np.array_equal(np.isnan(ref[:, 0]), outside)            # the reference: answered on the first and last line, not beyond
    out = q(M, "rest", xz, 0)
    assert np.array_equal(np.isnan(out).all(1), outside) and np.array_equal(np.isnan(out).any(1), outside)
    a, r = out[~outside], ref[~outside]
    assert np.abs(a[:, :3] - r[:, :3]).max() <= 1e-5 * float(np.abs(M.vert).max())
    assert np.abs(a[:, 3:6] - r[:, 3:6]).max() <= 1e-5
    assert np.abs(a[:, 6] - r[:, 6]).max() <= 1e-5 * max(1.0, float(M.white.max()))
    assert (a[:, 7] == 0).all()


# ---- world mode --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def feature_points(R, uw, fold):
    xz = S.displaced_feature_points(mesh(R, uw, fold).vert, R)
    xz.setflags(write=False)
    return xz


def world_features(q, M, iters, vel_of=None):
    """Vertices, edge midpoints and diagonal midpoints of an unfolded mesh.  Where a triangle holds the point (containing, tol 1e-6; on an
    edge several do, and agree): its height, normal and whitecap, residual ~0.  The border midpoints that rounded off the footprint: a
    point of the mesh with an honest residual.  vel_of(rows) -> vout rows of the same call, held to the triangle's velocity.
    -> (largest height error / scale, largest residual / uw, points off the footprint)"""
    xz = feature_points(M.R, M.uw, M.fold)
    out = q(M, "world", xz, iters)
    assert np.isfinite(out).all()
    count, _, ref, vref = S.world_reference(xz, out[:, 1], M.vert, M.norm, M.white, M.R, M.uw, 1e-6, vel=M.vel)
    on = count > 0
    assert on.sum() >= len(xz) - 4 * (M.R - 1)                       # only border midpoints can round off the footprint
    dy = np.abs(out[on, 1] - ref[on, 1])
    assert dy.max() <= 1e-5 * M.scale, (dy.max() / M.scale, xz[on][dy.argmax()])
    assert out[on, 7].max() <= 1e-4 * M.uw, (out[on, 7].max() / M.uw, xz[on][out[on, 7].argmax()])
    assert np.abs(out[on, 3:6] - ref[on, 3:6]).max() <= 1e-4
    assert np.abs(out[on, 6] - ref[on, 6]).max() <= 1e-4 * M.wscale
    if (~on).any():
        assert_on_mesh_and_honest(out[~on], xz[~on], M)
    if vel_of is not None:
        vmax = float(np.abs(M.vel).max())
        np.testing.assert_allclose(vel_of()[on, :3], vref[on], rtol=1e-6, atol=2e-5 * vmax)
    return float(dy.max() / M.scale), float(out[on, 7].max() / M.uw), int((~on).sum())


def tiny_points(M, n=400, seed=5):
    """n points strictly inside random displaced triangles of M (barycentric weights >= 1e-3)"""
    rng = np.random.default_rng(seed)
    tris = S.grid_triangles(M.R)
    t = tris[rng.integers(0, len(tris), n)]
    w = 1e-3 + (1.0 - 3e-3) * rng.dirichlet(np.ones(3), n)
    return (w[..., None] * M.vert[:, [0, 2]].astype(np.float64)[t]).sum(1).astype(np.float32)


def world_tiny(q, M):
    xz = tiny_points(M)
    out = q(M, "world", xz, 0)
    nuniq, nfold, _ = S.check_world(out, xz, M.vert, M.norm, M.white, M.uw, S.all_triangles(M.R), unique_exact=True)
    assert nfold == 0 and nuniq == len(xz) == 400, (nuniq, nfold)


def off_footprint(q, M, xz, iters=0):
    """World points off the displaced footprint: the best visited point of the clamped walk -- a point of the mesh, its honest distance,
    never nearer than the border.  -> (out, largest (residual - border distance) / uw)"""
    out = q(M, "world", xz, iters)
    assert_on_mesh_and_honest(out, xz, M)
    bd = S.border_distance(xz, M.vert, M.R)
    _, bound = _honest(out, xz)
    assert (out[:, 7] >= bd - bound).all(), (out[:, 7] - bd).min()
    return out, float(((out[:, 7] - bd) / M.uw).max())


@functools.lru_cache(maxsize=None)
def ring(R, uw, fold, dist, n=2000):
    xz = S.off_footprint_ring(mesh(R, uw, fold).vert, R, uw, dist, n)
    xz.setflags(write=False)
    return xz


# ---- iterations --------------------------------------------------------------------------------------------------------------------
def iteration_points(M, n=3000, seed=6):
    rc = S.rest_coords(M.R, M.uw)
    return np.random.default_rng(seed).uniform(float(rc[0]) - 6 * M.uw, float(rc[-1]) + 6 * M.uw, (n, 2)).astype(np.float32)


def iterations(q):
    """More iterations never leave a point worse off (beyond the `resolved` threshold: an early exit recomputes its residual), and
    iterations = 0 is iterations = 8."""
    M = mesh(32, 1.0, 2.5, seed=3 + 32)
    xz = iteration_points(M)
    res = {it: q(M, "world", xz, it) for it in ITER_COUNTS + (0,)}
    for a, b in zip(ITER_COUNTS, ITER_COUNTS[1:]):
        grow = res[b][:, 7] - res[a][:, 7]
        assert np.isfinite(res[b]).all() and grow.max() <= 1e-4 * M.uw, (a, b, grow.max(), xz[grow.argmax()])
    assert np.array_equal(res[0].view(np.uint32), res[DEFAULT_ITERS].view(np.uint32))


# ---- defective vertices ------------------------------------------------------------------------------------------------------------
DEFECT_AT = (10, 10)


@functools.lru_cache(maxsize=None)
def defective(kind):
    """mesh(128, 1.0, 0.9) with vertex (10, 10) NaN, +inf in x, or the lower triangle of cell (10, 10) collapsed onto it (its two other
    corners (11, 10) and (10, 11) moved to its position: a zero-area triangle with zero-length edges).  -> (vert, ids of the moved or
    broken vertices)"""
    M = mesh(128, 1.0, 0.9)
    v = M.vert.copy()
    c = DEFECT_AT[0] * M.R + DEFECT_AT[1]
    ids = [c]
    if kind == "nan":
        v[c] = np.nan
    elif kind == "inf_x":
        v[c, 0] = np.inf
    else:
        ids = [c, c + M.R, c + 1]
        v[c + M.R] = v[c]
        v[c + 1] = v[c]
    v.setflags(write=False)
    return v, np.array(ids)


def defect_points(n=20000, seed=8):
    M = mesh(128, 1.0, 0.9)
    rc = S.rest_coords(M.R, M.uw)
    return np.random.default_rng(seed).uniform(float(rc[0]), float(rc[-1]), (n, 2)).astype(np.float32)


def defects(q, kind, iters):
    """One broken vertex spoils no answer away from it.  Every row stays finite, on the mesh's sound triangles, with an honest residual.
    The walk of the clean mesh visits rest points within iters * MW_SQ_MAX_STEP cells of its start (the query) and reads vertices one
    cell further; its answer lies within the largest displacement dmax of the query's neighbourhood: a clean answer further than
    iters * MW_SQ_MAX_STEP + ceil(dmax / uw) + 2 cells (on either axis) from the broken vertices never read them, and keeps its bits.
    -> (rows held to the clean bits, rows that differ from the clean mesh)"""
    M = mesh(128, 1.0, 0.9)
    vert, ids = defective(kind)
    xz = defect_points()

    class D:   # the mesh q sees
        R, uw, fold, norm, white, vel = M.R, M.uw, M.fold, M.norm, M.white, M.vel
    D.vert = vert
    out, clean = q(D, "world", xz, iters), q(M, "world", xz, iters)
    # the reference mesh: a non-finite vertex belongs to no triangle a finite answer can lie on
    sound = np.where(np.isfinite(vert).all(-1)[:, None], vert, np.nan)
    assert_on_mesh_and_honest(out, xz, M, vert=sound)
    eff = DEFAULT_ITERS if iters == 0 else iters
    dmax = float(np.abs(M.vert[:, [0, 2]] - S.rest_plane(M.R, M.uw)).max())
    cells = eff * MAX_STEP + math.ceil(dmax / M.uw) + 2
    at = S.rest_plane(M.R, M.uw)[ids].astype(np.float64)
    far = (np.abs(clean[:, None, [0, 2]].astype(np.float64) - at[None]).max(-1) > cells * M.uw).all(1)
    same = (out.view(np.uint32) == clean.view(np.uint32)).all(1)
    assert same[far].all(), (kind, iters, xz[far & ~same][:5])
    return int(far.sum()), int((~same).sum())
