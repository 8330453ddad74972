"""CPU tier of draught (mw_ocean_set_draught, include/mistral_water.h; csrc/hull_draught.h): the hull family on the water column.

The MW_HD functions built with g++ (tests/draught_shim.cpp: hull_vertex_draught, then the rows in the kernels' summation order) against
* Archimedes on flat water (hull_ref.submerged);
* the Smith effect: under one deep-water component the heave force on a spar of draught T falls off as e^{-kT};
* the float64 composition of the column's and the hull forces' references (tests/draught_ref.py) on the oracle's layers;
* the rows that have no answer, and a heaving box on flat water.
The bound of a row is the project's for hull forces: 1e-4 of the sum over the triangles of |F_t| or |tau_t|, and of
the wetted area for the area."""
import ctypes as C

import numpy as np
import pytest

import body_ref as B
import column_ref as CR
import draught_ref as DR
import hull_ref as H
import periodic_ref as PR
import surface_ref as S
import workloads

f32 = np.float32
RHO, G = DR.RHO, DR.G
REL = 1e-4   # of S (hull_ref.term_scales), DESIGN.md section 7d
R64, UW = 64, 1.0
FLAT_DEPTHS = np.array([0.0, 4.0, 8.0, 16.0], f32)


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return DR.build_shim(str(tmp_path_factory.mktemp("draught") / "libdraught_shim.so"))


@pytest.fixture(scope="module")
def surface_shim(tmp_path_factory):
    """the hull family without draught (tests/periodic_shim.cpp): the denominator of the Smith ratio"""
    return PR.build_shim(str(tmp_path_factory.mktemp("draught_ps") / "libperiodic_shim.so"))


@pytest.fixture(scope="module")
def flat():
    pos, vel = DR.flat_layers(R64, UW, 4)
    pos.setflags(write=False)
    vel.setflags(write=False)
    return pos, vel


def icosphere():
    return H.icosphere(1.5, 2)


def assert_rows(got, want, scales, tag):
    """rows [n, 7 or 8] float32 against float64 rows [n, 7] within REL of (S_F, S_tau, area) [n, 3]; returns the largest error / S"""
    got = np.asarray(got, np.float64)
    assert np.isfinite(got[:, :7]).all(), tag
    eF = np.abs(got[:, 0:3] - want[:, 0:3]).max(1) / scales[:, 0]
    eT = np.abs(got[:, 4:7] - want[:, 4:7]).max(1) / scales[:, 1]
    eA = np.abs(got[:, 3] - want[:, 3]) / scales[:, 2]
    worst = (float(eF.max()), float(eT.max()), float(eA.max()))
    print(tag, "max error / S: F %.3g  tau %.3g  area %.3g" % worst)
    assert eF.max() <= REL and eT.max() <= REL and eA.max() <= REL, (tag, worst)
    return worst


# ---- 1. Archimedes on flat water ------------------------------------------------------------------------------------------------------
def test_archimedes_on_flat_water(shim, flat):
    """Flat layers at depths (0, 4, 8, 16): the column's rest depth is -y (interpolated between flat layers, continued below the deepest),
    so a closed hull gets rho g V_sub upward through its centre of buoyancy.  Measured here: F_y is off rho g V by 4.4e-8 S_F
    (spar) and at most 3.2e-7 S_F (icosphere, three heights); the horizontal force is at most 7.5e-9 S_F, the torque about the centre
    of buoyancy 2.3e-9 S_tau (spar) and at most 4.1e-6 S_tau (icosphere)."""
    pos, vel = flat
    cases = [("spar", DR.spar(), [3.3, 0.0, -7.1], None)]
    rng = np.random.default_rng(1)
    for y in (0.6, 0.0, -0.9):
        cases.append(("icosphere y=%g" % y, icosphere(), [-11.2, y, 5.4], H.random_quaternions(1, rng)))
    for tag, (hull, tris), p, q in cases:
        body = DR.pack([p], q)
        _, rows = DR.forces(shim, R64, UW, 0.0, FLAT_DEPTHS, pos, vel, hull, tris, body, DR.coeffs())
        x = H.transform(body, hull)[0]
        V, cb = H.submerged(x, tris)
        if tag == "spar":
            assert abs(V - 32.0) < 1e-9 and abs(RHO * G * V - 313920.0) < 1e-6
        _, scales, _ = DR.forces_f64(R64, UW, 0.0, FLAT_DEPTHS, pos, vel, hull, tris, body, DR.coeffs())
        SF, St = scales[0, 0], scales[0, 1]
        F, tau = rows[0, 0:3].astype(np.float64), rows[0, 4:7].astype(np.float64)
        tau_cb = tau - np.cross(cb - body[0, 0:3].astype(np.float64), F)
        print(tag, "(Fy - rho g V) / S_F %.3g   |F_h| / S_F %.3g   |tau_cb| / S_tau %.3g" %
              ((F[1] - RHO * G * V) / SF, np.abs(F[[0, 2]]).max() / SF, np.abs(tau_cb).max() / St))
        assert abs(F[1] - RHO * G * V) <= REL * SF, tag
        assert np.abs(F[[0, 2]]).max() <= REL * SF, tag
        assert np.abs(tau_cb).max() <= REL * St, tag
        assert rows[0, 7] >= 0 and rows[0, 7] < 1e-5


# ---- 2. the Smith effect ---------------------------------------------------------------------------------------------------------------
def half_range(fy):
    return (np.max(fy) - np.min(fy)) / 2


@pytest.mark.parametrize("depths", [(0.0, 4.0, 8.0, 16.0), (0.0, 8.0, 16.0)], ids=["L4", "L3"])
@pytest.mark.parametrize("m", [2, 4])
def test_smith_effect(shim, surface_shim, m, depths):
    """One deep-water component, k = 2 pi m / 64, a = 0.05, on the periodic 64 x 64 mesh; the spar (draught T = 8) at 16 phases over one
    period, drag off.  The half range of F_y with the column's depths over the half range with eta - y must be e^{-kT} to 2 %: kT = pi / 2
    (m = 2) and pi (m = 4).  The float64 reference stays within 0.10 % and 0.09 % with layers (0, 4, 8, 16) and 0.19 % and 0.28 % with
    (0, 8, 16); the 2 % leaves room for the layer interpolation ((kD)^2 / 8) and float32."""
    hull, tris = DR.spar()
    body = DR.pack([[0.37, 0.0, -1.2]])
    P = PR.period(R64, UW)
    cf = DR.coeffs()
    fy = {k: [] for k in ("col64", "surf64", "col32", "surf32")}
    for j in range(16):
        pos, vel, k = DR.one_wave_layers(R64, UW, depths, m, 0.05, 2 * np.pi * j / 16)
        pos32, vel32 = pos.astype(f32), vel.astype(f32)
        fy["col64"].append(DR.forces_f64(R64, UW, P, depths, pos, vel, hull, tris, body, cf)[0][0, 1])
        fy["surf64"].append(DR.forces_f64(R64, UW, P, depths, pos, vel, hull, tris, body, cf, depth="surface")[0][0, 1])
        fy["col32"].append(float(DR.forces(shim, R64, UW, P, depths, pos32, vel32, hull, tris, body, cf)[1][0, 1]))
        fy["surf32"].append(float(PR.hull_forces(surface_shim, R64, UW, P, pos32[0], None, hull, tris, body, cf)[1][0, 1]))
    want = np.exp(-k * DR.SPAR_DRAUGHT)
    r64 = half_range(fy["col64"]) / half_range(fy["surf64"])
    r32 = half_range(fy["col32"]) / half_range(fy["surf32"])
    print("m %d  L %d  e^-kT %.5f  float64 %.5f (%.3f %%)  shim %.5f (%.3f %%)" % (m, len(depths), want, r64, 100 * (r64 / want - 1), r32, 100 * (r32 / want - 1)))
    assert half_range(fy["surf64"]) > 0.5 * RHO * G * 4.0 * 0.05   # the surface does heave the spar: about rho g a times the 2 x 2 bottom
    assert abs(r64 - want) <= 0.02 * want
    assert abs(r32 - want) <= 0.02 * want


# ---- 3. the shim against float64 on the oracle's layers ----------------------------------------------------------------------------------
N64, T64, DEPTHS64 = 64, 1.25, np.array([0.0, 2.0, 6.0, 18.0], f32)


@pytest.fixture(scope="module")
def layers(oracle):
    """the oracle's layers of section 7j's setup (N = 64, choppiness 0.46, L = 4), cast to float32: computed once, shared, never written"""
    p = workloads.fftmesh_params(N64)
    h0, h0c = oracle.generate_spectrum(p, 7)
    pos, vel = CR.layers_f64(p, h0, h0c, T64, DEPTHS64)
    pos, vel = pos.astype(f32), vel.astype(f32)
    pos.setflags(write=False)
    vel.setflags(write=False)
    return pos, vel


def poses(layers, P, seed, sunk_from, sunk_to):
    """24 poses afloat (hull_ref.afloat_poses: near the surface, upright within 15 degrees, random velocities) and 6 sunk ones between the
    given heights; on the tiling the last afloat pose and half the sunk ones lie in other tiles"""
    pos, _ = layers
    rng = np.random.default_rng(seed)
    rc0 = float(S.rest_coords(N64, UW)[0])

    def eta(xz):
        xz = np.asarray(xz, np.float64)
        if P:
            xz = np.mod(xz - rc0, P) + rc0
        return CR.layer_heights_f64(N64, UW, P, DEPTHS64[:1], pos[:1], xz)[0]

    p, q = H.afloat_poses(24, rng, 24.0, eta, tile_shift=(2 * P, -P) if P else None)
    ps = np.stack([rng.uniform(-24, 24, 6), rng.uniform(sunk_from, sunk_to, 6), rng.uniform(-24, 24, 6)], 1)
    if P:
        ps[::2, 0] += 3 * P
        ps[::2, 2] -= 2 * P
    p = np.concatenate([p, ps.astype(f32)])
    q = np.concatenate([q, H.upright_quaternions(6, rng)])
    return DR.pack(p, q, rng.standard_normal((30, 3)) * 0.8, rng.standard_normal((30, 3)) * 0.3)


@pytest.mark.parametrize("P", [0.0, 64.0], ids=["footprint", "tiling"])
@pytest.mark.parametrize("drag", [False, True], ids=["nodrag", "drag"])
@pytest.mark.parametrize("name", ["spar", "icosphere"])
def test_shim_equals_float64_on_oracle_layers(shim, layers, name, drag, P):
    """Every row within 1e-4 S of the float64 composition, no body left out.  Measured here (max error / S over the 30 bodies, the worst
    of the eight cases): F 4.8e-7, tau 5.6e-6, area 2.7e-6."""
    pos, vel = layers
    hull, tris = DR.spar() if name == "spar" else icosphere()
    # sunk: every vertex below layer 2 (rest depth 6; the layer's own motion is below 0.1 there)
    bodies = poses(layers, P, 5, *((-24.0, -15.5) if name == "spar" else (-21.0, -8.0)))
    cf = DR.coeffs(linear_drag=30.0, quadratic_drag=60.0, velocity_scale=0.5) if drag else DR.coeffs()
    slab, rows = DR.forces(shim, N64, UW, P, DEPTHS64, pos, vel, hull, tris, bodies, cf)
    want, scales, res = DR.forces_f64(N64, UW, P, DEPTHS64, pos, vel, hull, tris, bodies, cf)
    assert np.isfinite(rows).all() and np.isfinite(want).all()
    x, col = DR.column_f64(N64, UW, P, DEPTHS64, pos, vel, hull, bodies)
    assert (col[24:, :, CR.LAMBDA] >= 2).all() and (col[24:, :, CR.LAMBDA] == 3).any()        # sunk: below layer 2, some below the deepest
    assert (col[:24, :, CR.DEPTH] > 0).any(1).all() and (col[:24, :, CR.DEPTH] < 0).any(1).all()   # afloat: every hull cuts the surface
    assert_rows(rows, want, scales, "%s drag=%d P=%g" % (name, drag, P))
    assert (rows[:, 7] >= 0).all() and np.abs(rows[:, 7] - res).max() <= 1e-4
    if not drag:
        assert (slab[:, :, 4:7] == 0).all()
    else:
        assert (slab[:, :, 4:7] != 0).any()


# ---- 4. rows without an answer -------------------------------------------------------------------------------------------------------
def test_rows_without_an_answer(shim, flat):
    pos, vel = flat
    hull, tris = DR.spar()
    cf = DR.coeffs(linear_drag=30.0)
    body = DR.pack([[1.0, 0.0, 2.0], [np.nan, 0.0, 0.0], [0.0, 30.0, 0.0], [4.0, -40.0, -3.0], [2.0, 0.0, 1.0]], v=np.full((5, 3), 0.1))
    body[4, 0:3] = [3e38, 0.0, 0.0]   # finite pose, a vertex that overflows: 3e38 + R h is not finite for h.x = +1
    big_hull = hull.copy()
    big_hull[:, 0] *= f32(1e38)
    slab, rows = DR.forces(shim, R64, UW, 0.0, FLAT_DEPTHS, pos, vel, hull, tris, body, cf)
    assert np.isfinite(rows[0]).all()
    assert np.isnan(rows[1]).all() and np.isnan(slab[1]).all()                       # a NaN pose
    assert (rows[2, :7] == 0).all() and np.isfinite(rows[2, 7]) and rows[2, 7] >= 0  # wholly in the air: nothing wet, a residual all the same
    assert (slab[2, :, 3] < 0).all() and (slab[2, :, 4:7] == 0).all()
    # wholly below the deepest layer (16): the hydrostatic continuation gives rho g V, with drag against still water
    V = H.volume(H.transform(body[3:4], hull)[0], tris)
    want, scales, _ = DR.forces_f64(R64, UW, 0.0, FLAT_DEPTHS, pos, vel, hull, tris, body[3:4], DR.coeffs())
    _, still = DR.forces(shim, R64, UW, 0.0, FLAT_DEPTHS, pos, vel, hull, tris, DR.pack([[4.0, -40.0, -3.0]]), DR.coeffs())
    assert (slab[3, :, 3] > 16).all() and abs(V - 64.0) < 1e-9
    assert abs(float(still[0, 1]) - RHO * G * V) <= REL * scales[0, 0] and np.abs(still[0, [0, 2]]).max() <= REL * scales[0, 0]
    assert abs(want[0, 1] - RHO * G * V) <= 1e-6 * RHO * G * V   # the coefficients are float32: 9.81f is 4e-8 off 9.81
    # a non-finite vertex
    _, r = DR.forces(shim, R64, UW, 0.0, FLAT_DEPTHS, pos, vel, big_hull, tris, body[4:5], cf)
    assert np.isnan(r).all()
    # a triangle index out of range: the row is NaN, nothing is read
    for bad in (-1, len(hull)):
        t = tris.copy()
        t[5, 1] = bad
        _, r = DR.forces(shim, R64, UW, 0.0, FLAT_DEPTHS, pos, vel, hull, t, body[0:1], cf)
        assert np.isnan(r).all()
    # and on the tiling the same rules
    _, rt = DR.forces(shim, R64, UW, 64.0, FLAT_DEPTHS, pos, vel, hull, tris, body, cf)
    assert np.isnan(rt[1]).all() and (rt[2, :7] == 0).all() and np.isfinite(rt[[0, 3]]).all()


# ---- 5. heave ------------------------------------------------------------------------------------------------------------------------
def test_heave_period_on_flat_layers(shim, flat):
    """The box of tests/test_bodies_gpu.py::test_heave_period (2 x 1 x 3, half the water's density, released 0.1 high, undamped), stepped
    through the shim on flat layers: the period from the downward zero crossings over 3 periods is 2 pi sqrt(m / (rho g A_wp)) to 1 %, that
    test's bound.  The column does not disturb hydrostatics."""
    pos, vel = flat
    hull, tris = H.box(2.0, 1.0, 3.0)
    m = 500.0 * 6.0
    I = B.box_inertia(m, 2.0, 1.0, 3.0)
    mass = np.array([[m, I[0, 0], I[1, 1], I[2, 2], 0, 0, 0, 0]], f32)
    T = 2 * np.pi * np.sqrt(m / (RHO * G * 6.0))
    b = DR.pack([[0.0, 0.1, 0.0]])
    dt, K = 0.008, 4
    ys, ts = [0.1], [0.0]
    while ts[-1] < 3.3 * T:
        b, _ = DR.step(shim, R64, UW, 0.0, FLAT_DEPTHS, pos, vel, hull, tris, b, mass, DR.coeffs(), dt, K)
        ys.append(float(b[0, 1]))
        ts.append(ts[-1] + dt)
    ys, ts = np.array(ys), np.array(ts)
    k = np.nonzero((ys[:-1] > 0) & (ys[1:] <= 0))[0]
    tc = ts[k] + (ts[k + 1] - ts[k]) * ys[k] / (ys[k] - ys[k + 1])
    assert len(tc) >= 3
    period = (tc[-1] - tc[0]) / (len(tc) - 1)
    print("heave period %.5f, closed form %.5f" % (period, T))
    assert abs(period - T) <= 0.01 * T, (period, T)
    assert 0.09 <= ys.max() <= 0.101 and -0.101 <= ys.min() <= -0.09


# ---- exports and statuses without a GPU --------------------------------------------------------------------------------------------
def test_draught_symbols_are_exported_declared_and_refuse_a_null_handle(mw):
    from mistral_water import _native
    L = C.CDLL(_native.LIB_PATH)
    hdr = open(_native.HEADER_PATH).read()
    for s in ("mw_ocean_set_draught", "mw_ocean_get_draught"):
        assert hasattr(L, s) and s in _native.ABI_SYMBOLS and s + "(" in hdr
    L = mw.lib()
    assert L.mw_abi_version() == 4
    for on in (0, 1, 2, -1):
        assert L.mw_ocean_set_draught(None, on) == mw.MW_EINVAL and b"NULL handle" in L.mw_last_error()
    on = C.c_int32(7)
    assert L.mw_ocean_get_draught(None, C.byref(on)) == mw.MW_EINVAL and on.value == 7
