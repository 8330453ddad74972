"""CPU tier of the raycasts (mw_ocean_raycast, include/mistral_water.h).

* the two entry points are exported, declared, and refuse bad arguments with a status without a GPU;
* the MW_HD functions of csrc/raycast.h compiled with g++ (tests/raycast_shim.cpp, strict float32): the hierarchy and its traversal
  against a brute force over every triangle with the same intersection, bit for bit, on flat, rough and folded meshes of 2 to 130
  vertices a side; watertightness; a float64 Möller–Trumbore (tests/ray_ref.py); agreement with the world-mode surface query; the rows
  of misses and invalid rays; facing; a ray alone against the same ray in a batch."""
import ctypes as C

import numpy as np
import pytest

import ray_ref as RR
import surface_ref as S


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return RR.build_shim(str(tmp_path_factory.mktemp("rc") / "librc_shim.so"))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_mesh = RR.synthetic   # flat (y = 0, horizontally displaced), rough (below the fold limit) or choppy (folded)


def _rays(m, seed, n):
    return np.concatenate(list(RR.families(m.vert, m.R, np.random.default_rng(seed), n=n).values()))


def _same(o1, h1, o2, h2):
    return (_bits(o1) == _bits(o2)).all(1) & (h1 == h2).all(1)


# ---- the ABI ------------------------------------------------------------------------------------------------------------
def test_raycast_symbols_exported_and_declared(mw):
    from mistral_water import _native
    L = C.CDLL(_native.LIB_PATH)
    for s in ("mw_ocean_raycast", "mw_ocean_raycast_device"):
        assert hasattr(L, s) and s in _native.ABI_SYMBOLS
    hdr = open(_native.HEADER_PATH).read()
    assert "mw_status mw_ocean_raycast(mw_ocean* o, int32_t frame, const float* rays, int64_t n, float* out, int32_t* hit);" in hdr


def test_raycast_bad_arguments_are_statuses(mw):
    """No handle can exist without a GPU: malformed calls are refused by status, never by a crash."""
    L = mw.lib()
    rays = np.zeros((4, 8), np.float32)
    out = np.zeros((4, 8), np.float32)
    hit = np.zeros((4, 2), np.int32)
    assert L.mw_ocean_raycast(None, -1, rays.ctypes.data, 4, out.ctypes.data, hit.ctypes.data) == mw.MW_EINVAL
    assert b"NULL handle" in L.mw_last_error()
    assert L.mw_ocean_raycast(None, -1, None, 0, None, None) == mw.MW_EINVAL
    assert L.mw_ocean_raycast_device(None, -1, rays.ctypes.data, 4, out.ctypes.data, None) == mw.MW_EINVAL
    assert L.mw_ocean_raycast_device(None, -1, rays.ctypes.data + 4, 4, out.ctypes.data, None) == mw.MW_EINVAL
    assert b"aligned" in L.mw_last_error()


# ---- the traversal is the brute force ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flat", "rough", "choppy"])
@pytest.mark.parametrize("R", [2, 3, 17, 64, 130])
def test_traversal_equals_brute_force_bit_for_bit(shim, R, kind):
    """The hierarchy prunes nothing that holds the first hit: t, the 7 outputs and hit equal the brute force's bits for every ray of
    every family, with leaf blocks of 1, 3, 8 and 16 cells (block counts 1 to 129 a side, powers of two and not).  Windows that cut
    off the nearest hit (tmin just past it, tmax just before it) are added from the brute force's own answers."""
    m = _mesh(R, kind, seed=R)
    rays = _rays(m, R + 1, 120 if R <= 64 else 50)
    ob, hb = RR.cast(shim, m, rays, brute=True)
    hitk = hb[:, 0] >= 0
    t1 = ob[hitk, 0]
    past, before = rays[hitk].copy(), rays[hitk].copy()
    past[:, 3], past[:, 7] = np.nextafter(t1, np.float32(np.inf)), np.inf
    before[:, 7] = np.nextafter(t1, np.float32(-np.inf))
    before = before[before[:, 7] >= before[:, 3]]
    rays = np.concatenate([rays, past, before])
    ob, hb = RR.cast(shim, m, rays, brute=True)
    assert hitk.sum() >= len(hitk) // 5, "the families must hit the mesh"
    n0 = len(hitk)
    assert ((hb[n0:n0 + len(t1), 0] < 0) | (ob[n0:n0 + len(t1), 0] > t1)).all()      # tmin past the nearest hit: a later one or none
    assert (hb[n0 + len(t1):, 0] < 0).all()                                          # tmax before it: none
    for B in (1, 3, 8, 16):
        ot, ht = RR.cast(shim, m, rays, B=B)
        bad = ~_same(ot, ht, ob, hb)
        assert not bad.any(), (B, int(bad.sum()), np.flatnonzero(bad)[:8], ot[bad][:3], ob[bad][:3], ht[bad][:3], hb[bad][:3])
    if kind == "choppy" and R >= 17:  # the folded mesh has overhangs: rays that cross the surface more than once
        tris = RR.id_triangles(R)
        multi = sum(int(np.isfinite(RR.triangle_t_f64(m.vert, tris, r)).sum() >= 3) for r in rays[:200])
        assert multi >= 5, multi


def test_hierarchy_node_count_and_empty_padding(shim):
    """An implicit complete quadtree over ceil((R-1)/B) leaves a side, padded to a power of two: padding leaves hold empty boxes, the
    root holds every vertex."""
    m = _mesh(130, "rough", seed=2)
    for B, D in ((8, 5), (16, 4), (3, 6), (129, 0)):
        nodes = shim.rc_shim_nodes(130, B)
        assert nodes == (4 ** (D + 1) - 1) // 3, (B, nodes)
        box = np.empty((nodes, 8), np.float32)
        assert shim.rc_shim_build(130, m.vert.ctypes.data, B, box.ctypes.data) == 0
        root = box[0]
        assert (root[0:3] <= m.vert.min(0)).all() and (root[4:7] >= m.vert.max(0)).all()
        S_ = 2 ** D
        leaves = box[(4 ** D - 1) // 3:].reshape(S_, S_, 8)
        nb = (130 - 2) // B + 1
        assert np.isinf(leaves[nb:, :, 0]).all() and np.isinf(leaves[:, nb:, 0]).all()
        assert np.isfinite(leaves[:nb, :nb]).all()


# ---- watertightness, the float64 reference, the surface query ---------------------------------------------------------------
@pytest.mark.parametrize("R,fold", [(17, 0.7), (64, 0.9)])
def test_watertight_vertical_rays_inside_the_footprint(shim, R, fold):
    """On an unfolded mesh every vertical ray strictly inside the displaced footprint hits, from above (facing +1) and from below
    (facing -1): rays through every interior vertex, through the midpoints of interior edges (the float32 midpoint may sit a hair to
    either side of the edge) and through random points of interior triangles."""
    vert, norm, white = S.synth_mesh(R, 1.0, fold, seed=3)
    m = RR.Mesh(R, vert, norm, white)
    V = m.vert.reshape(R, R, 3)
    inner = V[1:-1, 1:-1].reshape(-1, 3)
    mids = [(V[1:-1, 1:-2] + V[1:-1, 2:-1]) / np.float32(2), (V[1:-2, 1:-1] + V[2:-1, 1:-1]) / np.float32(2),
            (V[2:-1, 1:-2] + V[1:-2, 2:-1]) / np.float32(2)]
    rng = np.random.default_rng(R)
    tris = RR.id_triangles(R)
    i, j = tris[:, 2] // R, tris[:, 2] % R - 1
    interior = tris[(i >= 1) & (i <= R - 3) & (j >= 1) & (j <= R - 3)]
    pick = interior[rng.integers(0, len(interior), 2000)]
    w = rng.dirichlet([1, 1, 1], len(pick)).astype(np.float32)
    inside = (w[:, :, None] * m.vert[pick]).sum(1)
    xz = np.concatenate([inner, *[a.reshape(-1, 3) for a in mids], inside])[:, [0, 2]]
    top, bottom = float(m.vert[:, 1].max()) + 5, float(m.vert[:, 1].min()) - 5
    down = RR.pack(np.c_[xz[:, 0], np.full(len(xz), top), xz[:, 1]], [0.0, -1.0, 0.0])
    up = RR.pack(np.c_[xz[:, 0], np.full(len(xz), bottom), xz[:, 1]], [0.0, 1.0, 0.0])
    od, hd = RR.cast(shim, m, down)
    ou, hu = RR.cast(shim, m, up)
    assert (hd[:, 0] >= 0).all(), int((hd[:, 0] < 0).sum())
    assert (hu[:, 0] >= 0).all(), int((hu[:, 0] < 0).sum())
    assert (hd[:, 1] == 1).all() and (hu[:, 1] == -1).all()
    np.testing.assert_array_equal(od[:, 1], xz[:, 0])        # a vertical ray keeps its x and z exactly
    np.testing.assert_array_equal(od[:, 3], xz[:, 1])


@pytest.mark.parametrize("R,kind", [(17, "rough"), (17, "choppy"), (64, "rough"), (64, "choppy")])
def test_against_float64_moller_trumbore(shim, R, kind):
    """t agrees with a float64 Möller–Trumbore over every triangle to a relative 1e-5 (of t, or of the ray's travel over one cell when
    the hit is closer than that), and the triangle is the reference's first one unless another hit lies within that tolerance."""
    m = _mesh(R, kind, seed=7)
    f = RR.families(m.vert, R, np.random.default_rng(70 + R), n=120)
    rays = np.concatenate([f["random"], f["vertical"], f["segments"], f["windows"]])
    out, hit = RR.cast(shim, m, rays)
    tris = RR.id_triangles(R)
    nhit = 0
    for k, r in enumerate(rays):
        t = RR.triangle_t_f64(m.vert, tris, r)
        best = t.min()
        if hit[k, 0] < 0:
            assert not np.isfinite(best), (k, best)
            assert out[k, 0] == np.inf
            continue
        nhit += 1
        tol = 1e-5 * max(best, m.uw / float(np.linalg.norm(r[4:7].astype(np.float64))))
        assert abs(float(out[k, 0]) - best) <= tol, (k, out[k, 0], best)
        assert hit[k, 0] == int(np.argmin(t)) or t[hit[k, 0]] <= best + tol, (k, hit[k, 0], int(np.argmin(t)))
    assert nhit >= len(rays) // 5


@pytest.mark.parametrize("R", [17, 64])
def test_vertical_ray_hits_the_triangle_the_world_query_locates(shim, R):
    """On an unfolded mesh a vertical down-ray at (x, z) hits the triangle the world-mode query (surface_query.h) locates there, and
    its py is the query's height to a relative 1e-5.  A point within the query's barycentric slack of an edge may be located in the
    neighbour: then the ray's triangle must hold the point within that slack too."""
    vert, norm, white = S.synth_mesh(R, 1.0, 0.8, seed=5)
    m = RR.Mesh(R, vert, norm, white)
    rc = S.rest_coords(R, 1.0)
    dmax = float(np.abs(m.vert[:, [0, 2]] - S.rest_plane(R, 1.0)).max())
    xz = np.random.default_rng(R).uniform(rc[0] + dmax + 1, rc[-1] - dmax - 1, (3000, 2)).astype(np.float32)
    q, tri = RR.query_world(shim, m, xz, iters=32)
    assert (q[:, 7] <= 1e-4).all() and (tri >= 0).all()
    out, hit = RR.cast(shim, m, RR.pack(np.c_[xz[:, 0], np.full(len(xz), m.vert[:, 1].max() + 5), xz[:, 1]], [0.0, -1.0, 0.0]))
    scale = float(np.abs(m.vert[:, 1]).max())
    np.testing.assert_allclose(out[:, 2], q[:, 1], rtol=1e-5, atol=1e-5 * scale)
    other = np.flatnonzero(hit[:, 0] != tri)
    tris = RR.id_triangles(R)
    for k in other:                                          # the ray's triangle holds the point within the query's slack
        P = m.vert[tris[hit[k, 0]]][:, [0, 2]].astype(np.float64)
        w = np.linalg.solve(np.vstack([P.T, np.ones(3)]), np.r_[xz[k].astype(np.float64), 1.0])
        assert w.min() >= -2e-5, (k, w)
    assert len(other) <= 0.01 * len(xz), len(other)


# ---- the contract's rows ------------------------------------------------------------------------------------------------------
def test_misses_and_invalid_rays(shim):
    m = _mesh(17, "rough", seed=1)
    top = float(m.vert[:, 1].max())
    miss = RR.pack([[0.0, top + 1, 0.0], [1e4, 0.0, 0.0], [0.0, top + 1, 0.0]], [[0.0, 1.0, 0.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0]],
                   tmax=[np.inf, np.inf, 0.5])                 # up from above, away from the mesh, a segment ending above the water
    out, hit = RR.cast(shim, m, miss)
    assert (out[:, 0] == np.inf).all() and np.isnan(out[:, 1:]).all() and (hit == [-1, 0]).all()
    nan, inf = np.nan, np.inf
    bad = [([nan, 0, 0], [0, -1, 0], 0, inf), ([inf, 0, 0], [0, -1, 0], 0, inf), ([0, 0, 0], [0, nan, 0], 0, inf),
           ([0, 0, 0], [0, -inf, 0], 0, inf), ([0, top + 1, 0], [0, 0, 0], 0, inf), ([0, top + 1, 0], [0, -1, 0], -1, inf),
           ([0, top + 1, 0], [0, -1, 0], 2, 1), ([0, top + 1, 0], [0, -1, 0], nan, inf), ([0, top + 1, 0], [0, -1, 0], 0, nan)]
    rays = np.concatenate([RR.pack(o, d, a, b) for o, d, a, b in bad])
    out, hit = RR.cast(shim, m, rays)
    assert np.isnan(out).all() and (hit == [-1, 0]).all()
    ok = RR.pack([0.0, top + 1, 0.0], [0.0, -1.0, 0.0], np.float32(-0.0), inf)       # -0 is not below 0: a valid ray
    assert RR.cast(shim, m, ok)[1][0, 0] >= 0


def test_facing_is_the_float64_definition(shim):
    """facing = +1 exactly where d . n_g < 0 in float64 (n_g written out from the header's P(i,j) definition in numpy), on every hit of
    every family on a folded mesh, where rays meet the surface from both sides."""
    m = _mesh(64, "choppy", seed=9)
    rays = _rays(m, 9, 300)
    out, hit = RR.cast(shim, m, rays)
    k = hit[:, 0] >= 0
    want, dn = RR.facing_f64(m.vert, 64, hit[k, 0], rays[k, 4:7])
    np.testing.assert_array_equal(hit[k, 1], want)
    assert (hit[k, 1] == 1).sum() > 10 and (hit[k, 1] == -1).sum() > 10
    assert (hit[k, 1][dn == 0] == -1).all()                  # a ray in the triangle's plane: "otherwise"


def test_upward_ray_from_under_the_surface_faces_minus_one(shim):
    vert, norm, white = S.synth_mesh(33, 1.0, 0.5, seed=4)
    m = RR.Mesh(33, vert, norm, white)
    xz = np.random.default_rng(4).uniform(-8, 8, (500, 2)).astype(np.float32)
    q, _ = RR.query_world(shim, m, xz)
    o = np.c_[xz[:, 0], q[:, 1] - 0.25, xz[:, 1]]             # a quarter metre under the water at (x, z)
    out, hit = RR.cast(shim, m, RR.pack(o, [0.0, 1.0, 0.0]))
    assert (hit[:, 0] >= 0).all() and (hit[:, 1] == -1).all()
    np.testing.assert_allclose(out[:, 0], 0.25, rtol=1e-4)


def test_a_ray_alone_gives_its_bits_in_a_batch(shim):
    m = _mesh(64, "choppy", seed=11)
    rays = _rays(m, 11, 20)
    ob, hb = RR.cast(shim, m, rays)
    perm = np.random.default_rng(0).permutation(len(rays))
    op, hp = RR.cast(shim, m, rays[perm])
    assert _same(op, hp, ob[perm], hb[perm]).all()
    for k in range(0, len(rays), 7):
        o1, h1 = RR.cast(shim, m, rays[k:k + 1])
        assert _same(o1, h1, ob[k:k + 1], hb[k:k + 1]).all(), k


def test_pack_rays_broadcasts_and_an_empty_batch_stays_empty():
    from mistral_water.ocean import Ocean
    assert Ocean.pack_rays(np.zeros((0, 3)), np.zeros((0, 3))).shape == (0, 8)     # raycast([], []) does nothing, as n == 0 does
    r = Ocean.pack_rays([1.0, 20.0, 2.0], [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0]], 0.5, [1.0, 2.0])
    assert r.shape == (2, 8) and (r[:, 0:3] == [1, 20, 2]).all() and (r[:, 3] == 0.5).all() and (r[:, 7] == [1, 2]).all()
    with pytest.raises(ValueError):
        Ocean.pack_rays(np.zeros((3, 3)), np.zeros((2, 3)))
