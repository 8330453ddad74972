"""CPU tier of the hull summation scheme at its size edges (csrc/hull_forces.h, rigid_bodies.h, fleet.h): 256-triangle chunks, a 64-lane
tree per wave, the four waves in order, one partial row per chunk, and a reduce in which lane l adds chunks l, l + 64, ... before a lane
tree.  The kernels that run it are device-only; tests/hull_order.h::body_row (built into tests/periodic_shim.cpp) restates its order by hand and is what the GPU tier
(tests/test_hull_sizes_gpu.py) compares bits with.  Here that restatement is itself checked, on the edge hulls of tests/hull_ref.py
(edge_hull: 255 / 256 / 257 triangles, 40 triangles on 600 vertices, 16 384 / 16 385 and 32 769 triangles, i.e. 1, 1, 2, 3, 64, 65 and
129 chunks), over the synthetic periodic mesh periodic_synth(64, 1.0, 0.5):

* the ordered float32 rows against the float64 reference fed the same vertex slab, within 1e-4 S, S = the sum over the triangles of the
  reference's per-triangle |F| (|tau|, area) -- a scale that exists for an open mesh;
* on the float64 reference alone: deleting any one sentinel (a triangle of area 18 at a slot where chunks, waves and reduce laps meet)
  moves the row by at least 100 x that bound, so the comparison above cannot miss a lost slot;
* the launch arithmetic: hull_chunks / fleet_chunks at the chunk edges, bodies_step_lds at the one-launch plan's LDS limit."""
import ctypes as C
import os

import numpy as np
import pytest

import hull_ref as H
import periodic_ref as PR
import shim_build
from conftest import REPO

RHO, G = 1000.0, 9.81
R, UW = 64, 1.0
TOL = 1e-4
# name -> (ntris, nverts, chunks)
HULLS = {"t255": (255, None, 1), "t256": (256, None, 1), "t257": (257, None, 2), "t40_v600": (40, 600, 3), "t16384": (16384, None, 64),
         "t16385": (16385, None, 65), "t32769": (32769, None, 129)}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return PR.build_shim(str(tmp_path_factory.mktemp("hs") / "libperiodic_shim.so"))


@pytest.fixture(scope="module")
def mesh():
    vert, norm, white, vel = PR.periodic_synth(R, UW, 0.5)
    return dict(vert=vert, norm=norm, white=white, vel=vel)


_hulls = {}


def hull_of(name):
    if name not in _hulls:
        ntris, nverts, _ = HULLS[name]
        _hulls[name] = H.edge_hull(ntris, nverts)
    return _hulls[name]


def poses(shim, mesh, P, n, seed):
    """n bodies afloat on the synthetic mesh (hull_ref.afloat_poses), moving and spinning; on the tiling the last one lies in the
    neighbouring tile (+P along x, -P along z)"""
    rng = np.random.default_rng(seed)
    eta = lambda xz: PR.query(shim, R, UW, P, mesh["vert"], mesh["norm"], mesh["white"], 1, 1, xz)[:, 1].astype(np.float64)  # noqa: E731
    p, q = H.afloat_poses(n, rng, 20.0, eta, tile_shift=(P, -P) if P else None)
    b = np.zeros((n, 16), np.float32)
    b[:, 0:3], b[:, 4:8] = p, q
    b[:, 8:11] = rng.standard_normal((n, 3))
    b[:, 12:15] = 0.3 * rng.standard_normal((n, 3))
    return b


def reference(slab, tris, body, lin, quad):
    """(row [7], per-triangle terms [T, 7]) of the float64 reference on a body's vertex slab [V, 8] = x y z d ux uy uz residual"""
    s = slab.astype(np.float64)
    return H.forces(s[:, 0:3], s[:, 3], s[:, 4:7], tris, body, RHO, G, lin, quad, terms=True)


def bounds(per):
    """the bound on the (F, area, tau) parts of a row: TOL x the sum of the per-triangle magnitudes"""
    sf, st = H.term_scales(per)
    return TOL * sf, TOL * per[:, 3].sum(), TOL * st


# ---- the helpers themselves ---------------------------------------------------------------------------------------------------
def test_edge_hulls_have_the_sizes_and_the_sentinels_the_table_names(shim):
    for name, (ntris, nverts, chunks) in HULLS.items():
        x, t = hull_of(name)
        assert len(t) == ntris and t.min() >= 0 and t.max() < len(x)
        assert nverts is None or len(x) == nverts
        assert shim.ps_hull_chunks(len(x), len(t)) == chunks, name
        xx = x.astype(np.float64)
        area = 0.5 * np.cross(xx[t[:, 1]] - xx[t[:, 0]], xx[t[:, 2]] - xx[t[:, 0]])
        slots = H.sentinel_slots(ntris)
        assert slots == [k for k in (0, 255, 256, 16383, 16384) if k < ntris - 1] + [ntris - 1]
        assert np.allclose(area[slots], [0.0, -18.0, 0.0])                        # wound outward: down
        rest = np.delete(np.linalg.norm(area, axis=1), slots)
        assert rest.max() < 0.6 and (name[1:3] not in ("16", "32") or rest.max() < 0.0045)
    x, t = hull_of("t257")
    assert len(x) < 255                                                           # the triangles set the chunk count
    x, t = hull_of("t40_v600")
    assert t.max() < 222 and len(x) - len(np.unique(t)) >= 560                    # 2 chunks without a triangle; unreferenced vertices
    assert (len(hull_of("t16385")[0]), len(hull_of("t32769")[0])) == (9230, 18032)


def test_the_vectorised_reference_is_the_loop():
    x, t = hull_of("t257")
    rng = np.random.default_rng(3)
    b = np.zeros(16)
    b[0:3], b[4:8], b[8:11], b[12:15] = [1.0, -0.2, 2.0], H.upright_quaternions(1, rng)[0], rng.standard_normal(3), rng.standard_normal(3)
    X = H.transform(b[None], x)[0]
    d = 0.8 * np.sin(1.3 * X[:, 0]) + 0.5 * np.cos(X[:, 2]) - X[:, 1] - 1.0
    u = rng.standard_normal(X.shape)
    nwet = (d[t] > 0).sum(1)
    assert all((nwet == k).sum() >= 10 for k in range(4))                         # every branch of the clip
    for lin, quad in ((0.0, 0.0), (30.0, 60.0)):
        loop = H.forces(X, d, u, t, b, RHO, G, lin, quad)
        row, per = H.forces(X, d, u, t, b, RHO, G, lin, quad, terms=True)
        assert per.shape == (len(t), 7) and np.abs(row - loop).max() <= 1e-12 * np.abs(loop).max()
        one = H.forces(X, d, u, t[100:101], b, RHO, G, lin, quad)
        assert np.abs(per[100] - one).max() <= 1e-12 * max(np.abs(one).max(), 1.0)


# ---- 1. the ordered shim against float64 --------------------------------------------------------------------------------------
@pytest.mark.parametrize("drag", [False, True], ids=["buoyancy", "drag"])
@pytest.mark.parametrize("tiled", [False, True], ids=["footprint", "tiling"])
@pytest.mark.parametrize("name", list(HULLS))
def test_ordered_shim_against_float64(shim, mesh, name, tiled, drag):
    hull, tris = hull_of(name)
    P = PR.period(R, UW) if tiled else 0.0
    bodies = poses(shim, mesh, P, 3, seed=len(name) + 7 * tiled)
    lin, quad = (30.0, 60.0) if drag else (0.0, 0.0)
    cf = np.array([RHO, G, lin, quad, 1.0], np.float32)
    slab, rows = PR.hull_forces(shim, R, UW, P, mesh["vert"], mesh["vel"], hull, tris, bodies, cf)
    assert np.isfinite(rows).all() and (rows[:, 3] > 0).all() and (rows[:, 7] <= 1e-3).all()
    if tiled:
        assert abs(bodies[2, 0]) > 40.0                                           # in the neighbouring tile
    for b in range(len(bodies)):
        ref, per = reference(slab[b], tris, bodies[b], lin, quad)
        bf, ba, bt = bounds(per)
        err = np.abs(rows[b, :7] - ref)
        print(name, tiled, drag, b, "err/bound F %.2e A %.2e tau %.2e" % (err[0:3].max() / bf, err[3] / ba, err[4:7].max() / bt))
        assert err[0:3].max() <= bf and err[3] <= ba and err[4:7].max() <= bt, (b, rows[b], ref)


def test_a_nan_vertex_nobody_references_makes_the_row_nan(shim, mesh):
    """every vertex is counted, referenced or not: the NaN rule of hull_row"""
    hull, tris = hull_of("t40_v600")
    bad = hull.copy()
    bad[-1, 1] = np.nan
    assert not (tris == len(hull) - 1).any()
    cf = np.array([RHO, G, 0.0, 0.0, 1.0], np.float32)
    for P in (0.0, PR.period(R, UW)):
        bodies = poses(shim, mesh, P, 3, seed=5)
        _, good = PR.hull_forces(shim, R, UW, P, mesh["vert"], mesh["vel"], hull, tris, bodies, cf)
        _, rows = PR.hull_forces(shim, R, UW, P, mesh["vert"], mesh["vel"], bad, tris, bodies, cf)
        assert np.isfinite(good).all() and np.isnan(rows).all()


# ---- 2. the test proves its own sensitivity -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(HULLS))
def test_deleting_a_sentinel_moves_the_reference_by_100_bounds(shim, mesh, name):
    hull, tris = hull_of(name)
    bodies = poses(shim, mesh, 0.0, 3, seed=len(name))
    for lin, quad in ((0.0, 0.0), (30.0, 60.0)):
        cf = np.array([RHO, G, lin, quad, 1.0], np.float32)
        slab, _ = PR.hull_forces(shim, R, UW, 0.0, mesh["vert"], mesh["vel"], hull, tris, bodies, cf)
        for b in range(len(bodies)):
            ref, per = reference(slab[b], tris, bodies[b], lin, quad)
            bf, ba, bt = bounds(per)
            for k in H.sentinel_slots(len(tris)):
                less, _ = reference(slab[b], np.delete(tris, k, 0), bodies[b], lin, quad)
                moved = np.abs(ref - less)
                print(name, b, k, "moved/bound F %.0f A %.0f tau %.0f" % (moved[0:3].max() / bf, moved[3] / ba, moved[4:7].max() / bt))
                assert moved[0:3].max() >= 100 * bf and moved[3] >= 100 * ba and moved[4:7].max() >= 100 * bt, (name, b, k)


# ---- 3. launch arithmetic -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fleet_shim(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("hs_fleet") / "libfleet_shim.so")
    L = shim_build.strict_f32(os.path.join(REPO, "tests", "fleet_shim.cpp"), path)
    L.fs_chunks.argtypes = [C.c_int, C.c_int]
    return L


def test_chunk_counts_at_the_edges(shim, fleet_shim):
    want = {255: 1, 256: 1, 257: 2, 16384: 64, 16385: 65}
    for n, chunks in want.items():
        for other in (3, 40, n - 1, n):                                           # the smaller count never matters
            for nverts, ntris in ((n, other), (other, n)):                        # more vertices than triangles, and fewer
                assert shim.ps_hull_chunks(nverts, ntris) == chunks, (nverts, ntris)
                assert fleet_shim.fs_chunks(nverts, ntris) == chunks, (nverts, ntris)


def test_the_one_launch_plan_ends_at_5088_rows_of_lds(shim):
    top = shim.ps_bodies_lds_max()
    assert top == 159 * 1024 == 5088 * 32
    assert shim.ps_hull_chunks(5068, 5120) == 20 and shim.ps_hull_chunks(5069, 5120) == 20
    assert shim.ps_bodies_step_lds(5068, 20) == top
    assert shim.ps_bodies_step_lds(5069, 20) == top + 32 > top
    assert shim.ps_bodies_step_lds(600, 3) == 603 * 32
