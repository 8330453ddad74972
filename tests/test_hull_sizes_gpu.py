"""GPU tier of the hull summation scheme at its chunk and launch-size edges (k_hull_vertices / k_hull_triangles / k_hull_reduce,
k_bodies_step with its LDS slab and partials, the k_fleet_* set) through the C ABI, on FFTMesh 64^2, unit_width 1, one frame.

The hulls are tests/hull_ref.py's edge hulls (255 / 256 / 257 triangles, 40 triangles on 600 vertices, 16 384 / 16 385 and 32 769
triangles: 1, 1, 2, 3, 64, 65 and 129 chunks) with sentinels -- triangles of area 18 beside cells of 0.0044 -- in the slots where chunks,
waves and reduce laps meet.  On the periodic handle (kernels built without contraction) every row and state equals the ordered g++
restatement (tests/periodic_shim.cpp) bit for bit; tests/test_hull_sizes_cpu.py checks that restatement against float64 and shows that
a lost sentinel moves a row by a thousand bounds.  On the one footprint (kernels built with contraction) rows are held to the float64
reference within 1e-4 S, S the sum of the reference's per-triangle magnitudes, and the two plans and the two forms to each other.
Further: 4 * 2^20 + 5 bodies (workgroups and waves striding over the work of a capped grid), the one-launch plan at its LDS limit
(nverts + nchunks = 5088) and one vertex above it, and a fleet table with all 32 hulls."""
import numpy as np
import pytest

import body_ref as B
import hull_ref as H
import periodic_ref as PR
import test_fleet_gpu as TF
import test_hull_forces_gpu as THF
import test_periodic_gpu as TP

pytestmark = pytest.mark.gpu
bits = PR.bits
RHO, G = 1000.0, 9.81
TOL = 1e-4
DRAG = dict(linear_drag=30.0, quadratic_drag=60.0)
# name -> (ntris, nverts, cells of the barge it is cut from (None: hull_ref.edge_base), chunks)
HULLS = {"t255": (255, None, None, 1), "t256": (256, None, None, 1), "t257": (257, None, None, 2), "t40_v600": (40, 600, None, 3),
         "t16384": (16384, None, None, 64), "t16385": (16385, None, None, 65), "t32769": (32769, None, None, 129),
         # the one-launch plan's LDS limit: nverts + nchunks = 5088 rows of 32 B = MW_BODIES_LDS_MAX, and one vertex more
         "v5068": (5120, 5068, (46, 46), 20), "v5069": (5120, 5069, (46, 46), 20)}
_hulls = {}


def hull_of(name):
    if name not in _hulls:
        ntris, nverts, cells, chunks = HULLS[name]
        x, t = H.edge_hull(ntris, nverts, cells)
        assert (max(len(x), len(t)) + 255) // 256 == chunks
        _hulls[name] = (x, t)
    return _hulls[name]


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return PR.build_shim(str(tmp_path_factory.mktemp("hsg") / "libperiodic_shim.so"))


def _sea(mw, periodic):
    o, m = TP._ocean(mw, "fft64")
    o.set_periodic(periodic)
    return o, m


def _coeffs(o, drag):
    kw = DRAG if drag else {}
    return kw, np.array([RHO, G, kw.get("linear_drag", 0.0), kw.get("quadratic_drag", 0.0), 1.0 / o.params.t_division], np.float32)


def _afloat(mw, o, n, seed, shift=None, span=20.0):
    """n moving, spinning bodies that keep an edge hull's bottom sheet wet (hull_ref.afloat_poses on the handle's own surface); shift:
    the last one is moved by it, into a neighbouring tile"""
    rng = np.random.default_rng(seed)
    eta = lambda xz: o.query_surface(np.ascontiguousarray(xz, np.float32), mode="world")[:, 1].astype(np.float64)  # noqa: E731
    p, q = H.afloat_poses(n, rng, span, eta, tile_shift=shift)
    return mw.pack_bodies(p, q, rng.standard_normal((n, 3)), 0.3 * rng.standard_normal((n, 3)))


def _device_forces(o, hull, tris, bodies, **kw):
    import torch
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (hull, tris, bodies)]
    d_o = torch.zeros((len(bodies), 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    o.hull_forces_device(d[0].data_ptr(), len(hull), d[1].data_ptr(), len(tris), d[2].data_ptr(), len(bodies), d_o.data_ptr(), **kw)
    o.synchronize()
    return d_o.cpu().numpy()


def _mass(mw, n, rng):
    """mass rows for edge hulls (open meshes have no volume of their own): a 6 x 1.5 x 6 box of 20 to 30 t"""
    m = rng.uniform(20000.0, 30000.0, n)
    return mw.pack_mass(m, np.array([B.box_inertia(k, 6.0, 1.5, 6.0) for k in m]))


# ---- 4. the periodic handle against the ordered shim --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t255", "t256", "t257", "t40_v600", "t40_v600_nan", "t16384", "t16385", "t32769"])
def test_periodic_rows_equal_the_ordered_shim_bit_for_bit(mw, shim, name):
    hull, tris = hull_of(name.replace("_nan", ""))
    nan = name.endswith("_nan")
    if nan:                                                     # the last vertex, which no triangle references
        hull = hull.copy()
        hull[-1, 2] = np.nan
        assert not (tris == len(hull) - 1).any()
    o, m = _sea(mw, True)
    with o:
        bodies = _afloat(mw, o, 5, seed=len(name), shift=(m["P"], -m["P"]))
        assert abs(bodies[4, 0]) > 40.0                         # one body in the neighbouring tile
        for drag in (False, True):
            kw, cf = _coeffs(o, drag)
            _, want = PR.hull_forces(shim, m["R"], m["uw"], m["P"], m["vert"], m["vel"], hull, tris, bodies, cf)
            rows = o.hull_forces(hull, tris, bodies, **kw)
            if nan:                                             # every vertex is counted, referenced or not: hull_row's NaN rule
                assert np.isnan(want).all() and np.isnan(rows).all()
            else:
                assert np.isfinite(rows).all() and (rows[:, 3] > 0).all()
            bad = np.nonzero((bits(rows) != bits(want)).any(1))[0]
            assert len(bad) == 0, (name, drag, bad, rows[bad[:2]], want[bad[:2]])
            assert np.array_equal(bits(_device_forces(o, hull, tris, bodies, **kw)), bits(want)), (name, drag)
            for b in range(len(bodies)):                        # a body alone: the bits it has in the batch
                assert np.array_equal(bits(o.hull_forces(hull, tris, bodies[b:b + 1], **kw)[0]), bits(rows[b])), (name, drag, b)


# ---- 5. bodies, both plans, against the ordered shim --------------------------------------------------------------------------
@pytest.mark.parametrize("name,nbodies", [("t257", 4), ("t40_v600", 4), ("v5068", 2), ("v5069", 2)])
def test_periodic_bodies_equal_the_ordered_shim_in_both_plans(mw, shim, name, nbodies):
    """4 substeps, drag on.  v5068 asks the one-launch plan for 162 816 B of dynamic LDS, the documented limit (a refused launch would
    be an error status here); v5069 is one row above it, where a forced plan 1 must step per substep instead.  Which plan ran is not
    visible through the ABI: the rows and the states are what is asserted."""
    hull, tris = hull_of(name)
    o, m = _sea(mw, True)
    with o:
        bodies = _afloat(mw, o, nbodies, seed=len(name) + 1, shift=(-m["P"], m["P"]))
        mass = _mass(mw, nbodies, np.random.default_rng(2))
        kw, cf = _coeffs(o, True)
        for plan in (1, 0, -1):                                 # -1: the built-in rule (one launch up to 3 chunks, per substep above)
            got, rows = TP._run_plan(mw, plan, lambda: o.step_bodies(hull, tris, bodies.copy(), mass, 0.2, substeps=4, return_forces=True, **kw))
            order = plan if plan >= 0 else int(HULLS[name][3] < 4)
            sb, sr = PR.step_bodies(shim, m["R"], m["uw"], m["P"], m["vert"], m["vel"], hull, tris, bodies, mass, cf, 0.2, 4, order)
            assert np.isfinite(got).all() and np.isfinite(rows).all() and (rows[:, 3] > 0).all()
            assert not np.array_equal(got[:, 0:3], bodies[:, 0:3])
            assert np.array_equal(bits(rows), bits(sr)), (name, plan, rows, sr)
            assert np.array_equal(bits(got), bits(sb)), (name, plan)


# ---- 6. the one footprint ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["t257", "t16385", "t32769"])
def test_footprint_rows_against_float64(mw, name):
    """The SqMesh kernels are built with contraction, so they are not bit-equal to the shim: the rows are held to the float64 reference
    fed the library's own query answers at the instance vertices, within 1e-4 S (S = the sum over the triangles of the reference's
    per-triangle |F|, area or |tau|) -- the bound of the CPU tier, where the float32 restatement sits three orders of magnitude inside
    it.  Also: the device form has the host form's bits."""
    hull, tris = hull_of(name)
    o, m = _sea(mw, False)
    with o:
        bodies = _afloat(mw, o, 4, seed=len(name) + 2)
        x = H.transform(bodies, hull).astype(np.float32)
        for drag in (False, True):
            kw, cf = _coeffs(o, drag)
            rows = o.hull_forces(hull, tris, bodies, **kw)
            assert np.isfinite(rows).all() and (rows[:, 3] > 0).all()
            assert np.array_equal(bits(_device_forces(o, hull, tris, bodies, **kw)), bits(rows)), (name, drag)
            d, u, _ = THF._water_at(o, x, drag=drag, vscale=float(cf[4]))
            for b in range(len(bodies)):
                ref, per = H.forces(x[b], d[b], u[b], tris, bodies[b], RHO, G, float(cf[2]), float(cf[3]), terms=True)
                sf, st = H.term_scales(per)
                err = np.abs(rows[b, :7] - ref)
                print(name, drag, b, "err/bound F %.2e A %.2e tau %.2e" % (err[0:3].max() / (TOL * sf), err[3] / (TOL * per[:, 3].sum()),
                                                                          err[4:7].max() / (TOL * st)))
                assert err[0:3].max() <= TOL * sf and err[3] <= TOL * per[:, 3].sum() and err[4:7].max() <= TOL * st, (b, rows[b], ref)


@pytest.mark.parametrize("name", ["t257", "v5068"])
def test_footprint_plans_have_the_same_bits(mw, name):
    hull, tris = hull_of(name)
    o, m = _sea(mw, False)
    with o:
        bodies = _afloat(mw, o, 4, seed=len(name) + 3)
        mass = _mass(mw, 4, np.random.default_rng(3))
        run = lambda: o.step_bodies(hull, tris, bodies.copy(), mass, 0.2, substeps=4, return_forces=True, **DRAG)  # noqa: E731
        a, ra = TP._run_plan(mw, 0, run)
        b, rb = TP._run_plan(mw, 1, run)
        assert np.isfinite(a).all() and np.isfinite(ra).all() and (ra[:, 3] > 0).all() and not np.array_equal(a[:, 0:3], bodies[:, 0:3])
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(ra), bits(rb))


# ---- 7. launch geometry -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "footprint"])
def test_four_million_bodies_repeat_their_pattern(mw, shim, periodic):
    """nbodies = 4 * 2^20 + 5 tetrahedra (one chunk each): the smallest count at which k_hull_reduce's waves take a second lap over the
    bodies, and k_hull_triangles' workgroups several over the (body, chunk) items, of grids capped at 2^20 workgroups.  bodies[k] =
    pattern[k % 1021], 1021 prime, so no lap lines up with the pattern: every row must be row k % 1021.  The same through fleet_forces
    with a one-hull table (k_fleet_triangles, k_fleet_reduce).  About 1 GB of device memory lives in the handle until it is freed."""
    hull, tris, _ = TF._shapes()[0]
    n, period = 4 * 2 ** 20 + 5, 1021
    rng = np.random.default_rng(11)
    span = 96.0 if periodic else 24.0                                           # 3 x 3 tiles, or inside the one footprint
    idx = np.arange(n) % period
    o, m = _sea(mw, periodic)
    with o:
        pos = np.stack([rng.uniform(-span, span, period), np.zeros(period), rng.uniform(-span, span, period)], 1).astype(np.float32)
        pos[:, 1] = o.query_surface(np.ascontiguousarray(pos[:, [0, 2]]), mode="world")[:, 1] + rng.uniform(-0.6, 0.6, period)
        pattern = mw.pack_bodies(pos, H.random_quaternions(period, rng), rng.standard_normal((period, 3)), rng.standard_normal((period, 3)))
        bodies = np.ascontiguousarray(pattern[idx])
        kw, cf = _coeffs(o, periodic)
        if periodic:
            _, want = PR.hull_forces(shim, m["R"], m["uw"], m["P"], m["vert"], m["vel"], hull, tris, pattern, cf)
        else:
            want = o.hull_forces(hull, tris, pattern, **kw)
        assert np.isfinite(want).all() and (want[:, 3] > 0).sum() > period // 2
        x, t, table = mw.pack_fleet([(hull, tris, n)])
        for call in ("hull", "fleet"):
            rows = o.hull_forces(hull, tris, bodies, **kw) if call == "hull" else o.fleet_forces(x, t, table, bodies, coeffs=cf)
            assert rows.shape == (n, 8)
            assert np.array_equal(bits(rows[:period]), bits(want)), call
            same = (bits(rows) == bits(want)[idx]).all(1)
            assert same.all(), (call, int((~same).sum()), np.nonzero(~same)[0][:8])
            del rows, same


# ---- 8. the full fleet table --------------------------------------------------------------------------------------------------
def _full_fleet(mw, o, m, periodic):
    """32 hulls cycling through the edge hulls, the tetrahedron and the box, 0 to 3 bodies each -- none at the first, a middle and the
    last table position -- with drag per hull"""
    shapes = TF._shapes()
    cycle = [hull_of("t255"), hull_of("t256"), hull_of("t257"), hull_of("t40_v600"), hull_of("t16385"), shapes[0][:2], H.box(1.5, 1.0, 2.0)]
    rng = np.random.default_rng(21)
    counts = rng.integers(1, 4, 32)
    counts[[0, 15, 31]] = 0
    hulls = [cycle[h % len(cycle)] + (int(counts[h]),) for h in range(32)]
    n = int(counts.sum())
    shift = (m["P"], m["P"]) if periodic else None
    bodies = _afloat(mw, o, n, seed=22, shift=shift)
    bodies[:, [3, 11, 15]] = rng.standard_normal((n, 3)).astype(np.float32)     # the spare floats pass through
    cf = np.zeros((32, 5), np.float32)
    cf[:, 0], cf[:, 1], cf[:, 4] = rng.uniform(800.0, 1100.0, 32), rng.uniform(9.0, 10.0, 32), rng.uniform(0.5, 1.5, 32)
    cf[:, 2], cf[:, 3] = rng.uniform(10.0, 40.0, 32), rng.uniform(10.0, 80.0, 32)
    cf[1::3, 2:4] = 0.0                                                         # a third of the hulls without drag
    return TF.Fleet(hulls, bodies, _mass(mw, n, rng), cf)


@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "footprint"])
def test_a_table_of_32_hulls_equals_the_single_hull_calls(mw, periodic):
    o, m = _sea(mw, periodic)
    with o:
        F = _full_fleet(mw, o, m, periodic)
        assert len(F.hulls) == 32 and [F.hulls[h][2] for h in (0, 15, 31)] == [0, 0, 0] and {nb for _, _, nb in F.hulls} == {0, 1, 2, 3}
        want = TF._single_forces(o, F)
        edge = np.concatenate([np.arange(len(F.bodies))[F.rows(h)] for h in range(32) if h % 7 < 5])
        assert np.isfinite(want).all() and (want[edge, 3] > 0).all()
        rows = TF._fleet_forces(o, mw, F)
        bad = np.nonzero((bits(rows) != bits(want)).any(1))[0]
        assert len(bad) == 0, (bad, rows[bad[:2]], want[bad[:2]])
        wb, wr = TF._single_step(o, F, 0.1, 2)
        b, r = TF._step_fleet(o, mw, F, 0.1, 2)
        assert np.isfinite(wb).all() and not np.array_equal(wb[:, 0:3], F.bodies[:, 0:3])
        bad = np.nonzero((bits(b) != bits(wb)).any(1) | (bits(r) != bits(wr)).any(1))[0]
        assert len(bad) == 0, (bad,)
