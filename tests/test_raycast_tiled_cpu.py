"""CPU tier of the tiled raycasts (mw_ocean_raycast_tiled, csrc/raycast_tiled.h): the g++ build of the MW_HD functions the kernel runs
per lane (tests/raycast_tiled_shim.cpp) on synthetic frames -- any N x N displacement of the rest grid tiles by construction.

The column walk must equal the brute force over every triangle of every window tile bit for bit; whole-tile translations must leave the
hit alone; the 3 x 3 tiling must be watertight across its seams; interior cells must agree with the one-footprint cast; the leaf size must
not matter; the statuses must be the header's; and a float64 view of the window confirms the reported hit is the first."""
import numpy as np
import pytest

import ray_ref as RR
import ray_tiled_ref as RT

MESHES = [(2, "rough", 1.0), (4, "flat", 1.0), (4, "folded", 1.0), (6, "rough", 0.75), (8, "big", 1.0), (8, "rough", 1.0),
          (16, "folded", 1.0), (16, "rough", 0.75), (30, "rough", 1.0), (30, "flat", 1.0)]
BLOCKS = (1, 2, 3, 8)
REACHES = (0, 1, 2)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return RT.build_shim(str(tmp_path_factory.mktemp("rct") / "librct_shim.so"))


@pytest.fixture(scope="module")
def one_shim(tmp_path_factory):
    return RR.build_shim(str(tmp_path_factory.mktemp("rc1") / "librc_shim.so"))


def _mesh(k):
    N, kind, uw = MESHES[k]
    return RT.synthetic(N, kind, k + 1, uw)


def test_the_walk_equals_the_brute_force_bit_for_bit(shim):
    """every mesh x reach x family x leaf size: (t, tile, id) and the whole row; the conditions below keep the comparison from passing
    on rays that see nothing"""
    fam_hits, valid, hits, other_tile, seam, out_of_reach, saw_h2 = {}, 0, 0, 0, 0, 0, False
    for k, (N, kind, uw) in enumerate(MESHES):
        m = _mesh(k)
        saw_h2 |= RT.root(shim, m)[2] == 2
        fam = RT.families(m, np.random.default_rng(100 + k), n=40 if N >= 16 else 80)
        for reach in REACHES:
            for name, rays in fam.items():
                bo, bh = RT.cast(shim, m, rays, reach, brute=True)
                for B in BLOCKS:
                    out, hit = RT.cast(shim, m, rays, reach, B=B)
                    ok = RT.same_rows(out, hit, bo, bh)
                    assert ok.all(), (N, kind, uw, reach, name, B, int((~ok).sum()), rays[~ok][:2], out[~ok][:2], hit[~ok][:2], bo[~ok][:2],
                                      bh[~ok][:2])
                h = bh[:, 0] >= 0
                fam_hits[name] = fam_hits.get(name, 0) + int(h.sum())
                valid += int(np.isfinite(bo[:, 0]).sum() + np.isposinf(bo[:, 0]).sum())
                hits += int(h.sum())
                K0 = np.floor((rays[:, [0, 2]].astype(np.float64) - m.x0) / m.P)
                other_tile += int((h & ((bh[:, 2] != K0[:, 0]) | (bh[:, 3] != K0[:, 1]))).sum())
                cell = bh[:, 0] >> 1
                seam += int((h & ((cell // N == N - 1) | (cell % N == N - 1))).sum())
                oor = hit[:, 0] == RT.OUT_OF_REACH
                assert not (oor & h).any()
                out_of_reach += int(oor.sum())
    assert saw_h2, "one mesh must overhang by more than a period"
    assert all(v > 0 for v in fam_hits.values()) and len(fam_hits) == 9, fam_hits
    assert hits >= 0.25 * valid, (hits, valid)
    assert other_tile > 0 and seam > 0 and out_of_reach > 0, (other_tile, seam, out_of_reach)


def test_whole_tile_translations_leave_the_hit_alone(shim):
    """P a power of two, origins on multiples of 2^-8: the origin moved by (m P, 0, m' P) reduces to the same o', so t, id, facing,
    normal and whitecap keep their bits, the tile moves by (m, m') and px, pz by the float32 sum with m P (the base origins lie in tile 0,
    where nothing is added)"""
    for N, kind in ((8, "rough"), (16, "folded")):
        m = RT.synthetic(N, kind, 7)
        rng = np.random.default_rng(N)
        n = 300
        o = np.round(rng.uniform([m.x0, -3, m.x0], [m.x0 + m.P, 4, m.x0 + m.P], (n, 3)) * 256) / 256
        o[:, [0, 2]] = np.clip(o[:, [0, 2]], m.x0 + 1 / 256, m.x0 + m.P - 1 / 256)
        d = rng.normal(size=(n, 3))
        out0, hit0 = RT.cast(shim, m, RR.pack(o, d), 2)
        assert (hit0[:, 0] >= 0).sum() > n // 4 and (hit0[hit0[:, 0] >= 0, 2:] != 0).any()
        P = np.float32(m.P)
        for mx, mz in [(a, b) for a in range(-3, 4) for b in range(-3, 4)] + [(1000, 1000), (1000, -3), (-1000, 2)]:
            o2 = o + [mx * m.P, 0.0, mz * m.P]
            assert (o2.astype(np.float32) == o2).all()
            out, hit = RT.cast(shim, m, RR.pack(o2, d), 2)
            h = hit0[:, 0] >= 0
            assert np.array_equal(hit[:, :2], hit0[:, :2]), (mx, mz)
            assert np.array_equal(RT.bits(out[:, [0, 2, 4, 5, 6, 7]]), RT.bits(out0[:, [0, 2, 4, 5, 6, 7]])), (mx, mz)
            assert np.array_equal(hit[h, 2], hit0[h, 2] + mx) and np.array_equal(hit[h, 3], hit0[h, 3] + mz)
            assert np.array_equal(out[h, 1], out0[h, 1] + np.float32(mx) * P) and np.array_equal(out[h, 3], out0[h, 3] + np.float32(mz) * P)


def test_the_tiling_is_watertight_across_its_seams(shim):
    """vertical rays through every vertex and every edge midpoint of 3 x 3 tiles -- seam lines and tile corners included -- on meshes that
    do not fold: no ray slips through"""
    for N, uw in ((4, 1.0), (8, 0.75), (16, 1.0)):
        m = RT.synthetic(N, "rough", 40 + N, uw)
        tv, wi, wj = RT.tile_triangles(m)
        pts = []
        for kx in (-1, 0, 1):
            for kz in (-1, 0, 1):
                c = RT.shifted(m, tv, kx + wi, kz + wj).astype(np.float64)       # [2 N^2, 3, 3]
                pts += [c.reshape(-1, 3), ((c + np.roll(c, 1, 1)) / 2).reshape(-1, 3)]
        p = np.concatenate(pts).astype(np.float32)
        rays = np.concatenate([RR.pack(np.c_[p[:, 0], np.full(len(p), 9.0), p[:, 2]], [0.0, -1.0, 0.0]),
                               RR.pack(np.c_[p[:, 0], np.full(len(p), -9.0), p[:, 2]], [0.0, 1.0, 0.0])])
        out, hit = RT.cast(shim, m, rays, 2)
        assert (hit[:, 0] >= 0).all(), (N, int((hit[:, 0] < 0).sum()), rays[hit[:, 0] < 0][:3])
        assert {-2, -1, 0, 1, 2} >= set(np.unique(hit[:, 2:])) and len(np.unique(hit[:, 2])) >= 3


def test_interior_cells_agree_with_the_one_footprint_cast(shim, one_shim):
    """no overhang: a vertical ray strictly inside the footprint of the interior cells meets the same triangle with the same t bits as
    rc_cast on the one mesh, and the tiled id is that id + 2 ai"""
    for N, uw in ((8, 1.0), (16, 0.75)):
        m = RT.synthetic(N, "rough", 60 + N, uw)
        lo, hi, h = RT.root(shim, m)
        r = RT.rest(N, uw).astype(np.float64)
        rng = np.random.default_rng(N)
        xz = rng.uniform(r[1], r[N - 2], (400, 2))                # displacement < half a cell: cells 1 .. N-3 at least, never the seam
        rays = RR.pack(np.c_[xz[:, 0], np.full(400, 7.0), xz[:, 1]], [0.0, -1.0, 0.0])
        out, hit = RT.cast(shim, m, rays, 1)
        so, sh = RR.cast(one_shim, RR.Mesh(N, m.vert, m.norm, m.white, uw=uw), rays)
        assert (sh[:, 0] >= 0).all()
        ai = (sh[:, 0] >> 1) // (N - 1)
        assert np.array_equal(RT.bits(out[:, 0]), RT.bits(so[:, 0]))
        assert np.array_equal(hit[:, 0], sh[:, 0] + 2 * ai) and np.array_equal(hit[:, 1], sh[:, 1]) and (hit[:, 2:] == 0).all()
        assert np.array_equal(RT.bits(out), RT.bits(so))


def test_the_bits_do_not_depend_on_the_leaf_size(shim):
    m = RT.synthetic(30, "folded", 3)
    rays = np.concatenate(list(RT.families(m, np.random.default_rng(5), n=60).values()))
    ref = RT.cast(shim, m, rays, 2, B=2)
    assert (ref[1][:, 0] >= 0).mean() > 0.25
    for B in (1, 3, 4, 7, 8, 30, 64):
        out, hit = RT.cast(shim, m, rays, 2, B=B)
        assert np.array_equal(RT.bits(out), RT.bits(ref[0])) and np.array_equal(hit, ref[1]), B


def test_statuses(shim):
    m = RT.synthetic(4, "flat", 1)                               # y = 0.25 everywhere, P = 4, footprint [-1.5, 2.5]
    # a level ray inside the (padded) height range but off the plane of the water sees nothing and runs out of the window
    lo, hi, _ = RT.root(shim, m)
    y = float(np.nextafter(np.float32(0.25), np.float32(1)))
    assert lo[1] < y < hi[1]
    out, hit = RT.cast(shim, m, RR.pack([0.0, y, 0.0], [1.0, 0.0, 0.0]), 2)
    assert hit[0].tolist() == [RT.OUT_OF_REACH, 0, 0, 0] and np.isposinf(out[0, 0]) and np.isnan(out[0, 1:]).all()
    out, hit = RT.cast(shim, m, RR.pack([0.0, y, 0.0], [1.0, 0.0, 0.0], 0.0, 6.0), 2)  # ends in the window: tile 1 of 2
    assert hit[0].tolist() == [-1, 0, 0, 0] and np.isposinf(out[0, 0]) and np.isnan(out[0, 1:]).all()
    out, hit = RT.cast(shim, m, RR.pack([0.0, 3.0, 0.0], [0.3, 1.0, 0.1]), 2)           # upward from above the surface
    assert hit[0].tolist() == [-1, 0, 0, 0] and np.isposinf(out[0, 0])
    bad = np.concatenate([RR.pack([0.0, 1.0, 0.0], [0.0, 0.0, 0.0]), RR.pack([0.0, 1.0, 0.0], [0.0, -1.0, 0.0], 2.0, 1.0),
                          RR.pack([np.nan, 1.0, 0.0], [0.0, -1.0, 0.0]), RR.pack([0.0, 1.0, 0.0], [0.0, -1.0, 0.0], -1.0),
                          RR.pack([4.0 * (2 ** 20 + 2), 1.0, 0.0], [0.0, -1.0, 0.0]), RR.pack([0.0, 1.0, -4.0 * (2 ** 20 + 2)], [0.0, -1.0, 0.0])])
    out, hit = RT.cast(shim, m, bad, 2)
    assert np.isnan(out).all() and (hit == [-1, 0, 0, 0]).all()
    out, hit = RT.cast(shim, m, RR.pack([4.0 * (2 ** 20 - 1), 1.0, 0.0], [0.0, -1.0, 0.0]), 0)   # the farthest tiles still answer
    assert hit[0, 0] >= 0 and hit[0, 2] in (2 ** 20 - 1, 2 ** 20)


# The largest deviations the shim shows on these meshes, measured with the g++ build (this test prints them): the reported point lies
# 1.18e-7 off its triangle's plane, relative to the distance travelled plus the point's magnitude; a float64 hit strictly inside a window
# triangle comes 3.7e-7 (relative t) before the reported one.  4x that is allowed for the rounding of other hosts.
PLANE_MEASURED, EARLIER_MEASURED = 1.18e-7, 3.7e-7


def test_float64_view_of_the_window(shim):
    """the random family with origins in tile 0: the reported point lies on the plane of the reported triangle instance, and no float64
    hit on any window triangle precedes the reported t"""
    worst_plane = worst_early = 0.0
    for k in (2, 5, 6, 8):
        N, kind, uw = MESHES[k]
        m = _mesh(k)
        rng = np.random.default_rng(k)
        n = 150
        o = rng.uniform([m.x0, -3, m.x0], [m.x0 + m.P, 4, m.x0 + m.P], (n, 3))
        rays = RR.pack(o, rng.normal(size=(n, 3)))
        reach = 1
        out, hit = RT.cast(shim, m, rays, reach)
        P, K = RT.window_triangles(m, reach)
        flat = P.reshape(-1, 3)
        tris = np.arange(len(flat)).reshape(-1, 3)
        assert (hit[:, 0] >= 0).sum() > n // 4
        for r, o_, h_ in zip(rays, out, hit):
            t64 = RR.triangle_t_f64(flat, tris, r, slack=-1e-6)      # hits strictly inside a triangle only
            first = t64.min()
            if h_[0] < 0:
                assert not np.isfinite(first), (k, r, first)
                continue
            row = np.flatnonzero((K[:, 0] == h_[2]) & (K[:, 1] == h_[3]) & (K[:, 2] == h_[0]))[0]
            a, b, c = P[row].astype(np.float64)
            nrm = np.cross(b - a, c - a)
            nrm /= np.linalg.norm(nrm)
            scale = np.linalg.norm(r[4:7].astype(np.float64)) * o_[0] + np.abs(o_[1:4]).max()
            worst_plane = max(worst_plane, abs(np.dot(o_[1:4].astype(np.float64) - a, nrm)) / scale)
            if np.isfinite(first):
                worst_early = max(worst_early, (o_[0] - first) / max(abs(first), 1e-3))
    print("float64 view: worst plane distance %.3g (allowed %.3g), worst earlier hit %.3g (allowed %.3g)"
          % (worst_plane, 4 * PLANE_MEASURED, worst_early, 4 * EARLIER_MEASURED))
    assert worst_plane <= 4 * PLANE_MEASURED and worst_early <= 4 * EARLIER_MEASURED
