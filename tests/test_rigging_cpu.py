"""CPU tier of the rigged fleets (mw_ocean_step_rigged / _device, include/mistral_water.h): the model of csrc/rigging.h through
tests/rig_shim.cpp (g++, strict float32) against the moorings' shim, itself and tests/rig_ref.py (numpy float64).

1. every target MW_RIG_ANCHOR (and targets NULL): rig_wrench has mooring_wrench's bits, K = 1 and 8, over taut, slack and empty slots;
2. a mirrored pair: F_i == -F_j and T_i == T_j bitwise over 10^4 random poses and velocities;
3. the snapshot: a 5-body chain stepped 8 substeps keeps its bits under every permutation of the body order, targets remapped;
4. the shim against float64: the line wrench M on random taut scenes, and the state of the tow on flat water (rig_ref.tow_scene: the
   scene of the GPU tier's float64 test, which holds the device to 4x the figures printed here);
5. validity: a bad target, a self target, a non-finite partner and an invalid slot each hold that body alone;
6. the entry points and the constant are exported, declared and bound.

Measured (this file's seeds): M against float64 1.69e-6 of S_F and 1.66e-6 of S_tau at worst; the tow's state after 16 x 8 substeps, relative
to each block's change over the run: p 2.52e-7, q 4.59e-6, v 4.11e-7, w 2.26e-5 (test 4 prints them)."""
import ctypes as C
import itertools
import os
import re

import numpy as np
import pytest

import hull_ref as H
import mooring_ref as M
import periodic_ref as PR
import rig_ref as RR
import shim_build
import surface_ref as S
import test_moorings_cpu as TC
from conftest import REPO
from test_moorings_cpu import ms  # noqa: F401  (the moorings shim, as a fixture)

SHIM = os.path.join(REPO, "tests", "rig_shim.cpp")
TOL_F, TOL_TAU = TC.TOL_F, TC.TOL_TAU  # the moorings' bounds on the wrench: a tow slot's arithmetic is an anchored slot's at both ends


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def load_shim(path):
    L = shim_build.strict_f32(SHIM, path)
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    L.rs_wrench.restype = L.rs_step.restype = None
    L.rs_wrench.argtypes = [vp, vp, vp, i, i, vp, vp, vp]
    L.rs_step.argtypes = [vp, vp, vp, vp, vp, vp, i, i, vp, f, vp, vp]
    return L


@pytest.fixture(scope="module")
def rs(tmp_path_factory):
    return load_shim(str(tmp_path_factory.mktemp("rig") / "librig_shim.so"))


@pytest.fixture(scope="module")
def ps(tmp_path_factory):
    return PR.build_shim(str(tmp_path_factory.mktemp("rigp") / "libperiodic_shim.so"))


def wrench(rs, bodies, lines, targets):
    """(M [n, 8], tension [n, K], state [n]) of the shim"""
    bodies, lines = np.ascontiguousarray(bodies, np.float32), np.ascontiguousarray(lines, np.float32)
    targets = None if targets is None else np.ascontiguousarray(targets, np.int32)
    n, K = lines.shape[:2]
    Mo, T, state = np.zeros((n, 8), np.float32), np.zeros((n, K), np.float32), np.zeros(n, np.int32)
    rs.rs_wrench(_p(bodies), _p(lines), _p(targets), K, n, _p(Mo), _p(T), _p(state))
    return Mo, T, state


def step(rs, bodies, rows, mass, lines, targets, g, h, wrench=None):
    """one rigged substep of the shim over the whole array, in place -> (tension [n, K], state [n]); g a scalar or [n]"""
    n, K = lines.shape[:2]
    assert bodies.dtype == np.float32 and bodies.flags.c_contiguous
    rows, mass, lines = (np.ascontiguousarray(a, np.float32) for a in (rows, mass, lines))
    targets = None if targets is None else np.ascontiguousarray(targets, np.int32)
    wrench = None if wrench is None else np.ascontiguousarray(wrench, np.float32)
    gs = np.ascontiguousarray(np.broadcast_to(np.float32(g), (n,)), np.float32)
    T, state = np.zeros((n, K), np.float32), np.zeros(n, np.int32)
    rs.rs_step(_p(bodies), _p(rows), _p(mass), _p(wrench), _p(lines), _p(targets), K, n, _p(gs), h, _p(T), _p(state))
    return T, state


def tow_lines(mw, rng, bodies, K, partners):
    """lines [n, K, 12], targets [n, K], kinds [n, K] and `along` [n, K] on random poses: slot s of body b tows to body partners[b, s].  A
    quarter of the slots empty, of the others half slack and half taut with a stretch of 20 % at least and a damping term of at most half
    the spring term, as test_moorings_cpu.random_scene draws them, so that the error measured is the arithmetic's and not how near zero
    T's subtraction lands.  along: the line runs within 0.3 |d| of its arm, where the torque's cross product cancels."""
    n = len(bodies)
    lines = mw.pack_lines(n, K)
    lines[:, :, 0:3] = rng.uniform(-1, 1, (n, K, 3))
    lines[:, :, 4:7] = rng.uniform(-1, 1, (n, K, 3))
    b = np.asarray(bodies, np.float64)
    own = np.broadcast_to(b[:, None, :], (n, K, 16))
    d, va = RR._point(own, lines[:, :, 0:3].astype(np.float64))
    dj, vb = RR._point(b[partners], lines[:, :, 4:7].astype(np.float64))
    r = b[partners][:, :, 0:3] + dj - own[:, :, 0:3] - d
    l = np.linalg.norm(r, axis=2)
    e = r / l[:, :, None]
    along = np.linalg.norm(np.cross(d, e), axis=2) < 0.3 * np.linalg.norm(d, axis=2)
    kind = rng.choice([M.EMPTY, M.SLACK, M.TAUT, M.TAUT], (n, K), p=[0.25, 0.375, 0.1875, 0.1875])
    L0 = l * np.where(kind == M.SLACK, rng.uniform(1.05, 1.5, (n, K)), rng.uniform(0.3, 0.8, (n, K)))
    k = rng.uniform(10.0, 1000.0, (n, K))
    closing = np.abs(np.einsum("nki,nki->nk", va - vb, e))
    c = rng.uniform(0.0, 0.5, (n, K)) * k * np.abs(l - L0) / np.maximum(closing, 0.2 * np.linalg.norm(va - vb, axis=2))
    lines[:, :, 3] = L0
    lines[:, :, 7] = np.where(kind == M.EMPTY, 0.0, k)
    lines[:, :, 8] = np.where(kind == M.EMPTY, 0.0, c)
    return lines, np.ascontiguousarray(partners, np.int32), kind, along


# ---- 1. anchors only: the moorings' bits --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8])
def test_anchored_slots_have_mooring_wrench_bits(mw, ms, rs, K):  # noqa: F811
    rng = np.random.default_rng(300 + K)
    bodies, lines = TC.random_scene(mw, rng, 20000, K)
    want, Tw, taut = TC.wrench(ms, bodies, lines)
    kinds = M.wrenches(bodies, lines)[2]
    for kind in (M.EMPTY, M.SLACK, M.TAUT):
        assert (kinds == kind).mean() >= 0.10, kind
    for targets in (None, np.full((len(bodies), K), RR.ANCHOR, np.int32)):
        got, T, state = wrench(rs, bodies, lines, targets)
        assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(T), _bits(Tw)) and np.array_equal(state, taut)
    assert (taut == 1).any() and (taut == 0).any()


# ---- 2. a mirrored pair ------------------------------------------------------------------------------------------------------------
def test_mirrored_pair_is_equal_and_opposite_to_the_bit(mw, rs):
    rng = np.random.default_rng(310)
    n = 10000
    bodies = mw.pack_bodies(rng.standard_normal((2 * n, 3)) * 5, H.random_quaternions(2 * n, rng), rng.standard_normal((2 * n, 3)) * 2,
                            rng.standard_normal((2 * n, 3)))
    lines, targets = mw.pack_lines(2 * n, 1), np.zeros((2 * n, 1), np.int32)
    hi, hj = rng.uniform(-1, 1, (n, 3)), rng.uniform(-1, 1, (n, 3))
    i, j = np.arange(0, 2 * n, 2), np.arange(1, 2 * n, 2)
    lines[i, 0, 0:3], lines[i, 0, 4:7], lines[j, 0, 0:3], lines[j, 0, 4:7] = hi, hj, hj, hi
    targets[i, 0], targets[j, 0] = j, i
    lines[:, 0, 7] = 1.0
    l = np.linalg.norm(RR.slots(bodies, lines, targets)[1], axis=2)[i, 0] + 0.0  # with L0 = 0 and k = 1: T = l
    lines[i, 0, 3] = lines[j, 0, 3] = l * rng.uniform(0.3, 1.2, n)
    lines[i, 0, 7] = lines[j, 0, 7] = rng.uniform(10.0, 1000.0, n)
    lines[i, 0, 8] = lines[j, 0, 8] = rng.uniform(0.0, 300.0, n)  # large enough to clamp some closing pairs at T = 0
    Mo, T, state = wrench(rs, bodies, lines, targets)
    assert np.array_equal(state[i], state[j]) and set(np.unique(state)) == {0, 1}
    assert np.array_equal(_bits(T[i]), _bits(T[j]))
    taut = state[i] == 1
    assert taut.mean() > 0.6 and (T[i][taut] > 0).mean() > 0.8 and (T[i][taut] == 0).any()
    assert np.array_equal(_bits(Mo[i][taut][:, 0:3]), _bits(-Mo[j][taut][:, 0:3]))
    assert (np.abs(Mo[i][taut][:, 0:3]).max(1) > 0).mean() > 0.8


# ---- 3. the snapshot ---------------------------------------------------------------------------------------------------------------
def _chain_scene(mw, rng, n=5):
    """n bodies in a chain along x, 3 apart: body b holds a mirrored line to b - 1 (slot 0) and to b + 1 (slot 1), slot 2 an anchor line"""
    pos = np.stack([3.0 * np.arange(n), rng.uniform(-0.2, 0.2, n), rng.uniform(-0.5, 0.5, n)], 1)
    bodies = mw.pack_bodies(pos, H.upright_quaternions(n, rng, 20.0), rng.standard_normal((n, 3)) * 0.4, rng.standard_normal((n, 3)) * 0.3)
    m, I = 900.0, np.diag([300.0, 500.0, 400.0])
    mass = np.repeat(mw.pack_mass(m, I), n, 0)
    lines, targets = mw.pack_lines(n, 3), np.full((n, 3), RR.ANCHOR, np.int32)
    for b in range(n - 1):
        RR.mirror(lines, targets, b, 1, b + 1, 0, rng.uniform(-0.4, 0.4, 3), rng.uniform(-0.4, 0.4, 3), 2.0, 8.0 * m, 1.5 * m)
    lines[:, 2, 0:3] = rng.uniform(-0.4, 0.4, (n, 3))
    lines[:, 2, 4:7] = pos + [0.0, -4.0, 1.0]
    lines[:, 2, 3], lines[:, 2, 7], lines[:, 2, 8] = 3.5, 5.0 * m, 0.5 * m
    rows = np.zeros((n, 8), np.float32)
    rows[:, 1] = m * 9.81 * rng.uniform(0.9, 1.1, n)  # a constant lift near the weight, and a little torque
    rows[:, 4:7] = rng.standard_normal((n, 3)) * 20.0
    wr = np.zeros((n, 8), np.float32)
    wr[:, 0:3], wr[:, 4:7] = rng.standard_normal((n, 3)) * 100.0, rng.standard_normal((n, 3)) * 30.0
    return bodies, mass, rows, wr, lines, targets


def test_the_order_of_the_bodies_changes_no_bit(mw, rs):
    rng = np.random.default_rng(320)
    bodies, mass, rows, wr, lines, targets = _chain_scene(mw, rng)
    n = len(bodies)

    def run(order):
        inv = np.argsort(order)  # old index -> new index
        b = np.ascontiguousarray(bodies[order])
        t = np.where(targets[order] >= 0, inv[np.maximum(targets[order], 0)], targets[order]).astype(np.int32)
        for _ in range(8):
            T, state = step(rs, b, rows[order], mass[order], lines[order], t, 9.81, 0.02, wr[order])
        out, To = np.empty_like(b), np.empty_like(T)
        out[order], To[order] = b, T
        return out, To, state
    want, Tw, state = run(np.arange(n))
    assert (state == 1).all() and (Tw[:, 2] > 0).all() and (Tw[1:, 0] > 0).any() and np.isfinite(want).all()
    for order in itertools.permutations(range(n)):
        got, T, _ = run(np.array(order))
        assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(T), _bits(Tw)), order
    # and a sequential update would differ: stepping body 0 first and letting body 1 see it moves body 1's bits
    seq = bodies.copy()
    for _ in range(8):
        for b in range(n):
            one = seq.copy()
            step(rs, one, rows, mass, lines, targets, 9.81, 0.02, wr)
            seq[b] = one[b]
    assert not np.array_equal(_bits(seq), _bits(want))


# ---- 4. against float64 ------------------------------------------------------------------------------------------------------------
def test_wrench_against_float64(mw, rs):
    rng = np.random.default_rng(330)
    n, K = 20000, 4
    bodies = mw.pack_bodies(rng.standard_normal((n, 3)) * 5, H.random_quaternions(n, rng), rng.standard_normal((n, 3)) * 2,
                            rng.standard_normal((n, 3)))
    partners = (np.arange(n)[:, None] + rng.integers(1, n, (n, K))) % n  # never the body itself
    lines, targets, kind, along = tow_lines(mw, rng, bodies, K, partners)
    # the last slot anchored where its partner's point stands, undamped (its damping was sized for the relative speed): both kinds in one sum
    pb = bodies[partners[:, K - 1]].astype(np.float64)
    lines[:, K - 1, 4:7] = pb[:, 0:3] + RR._point(pb, lines[:, K - 1, 4:7].astype(np.float64))[0]
    lines[:, K - 1, 8] = 0.0
    lines[:, K - 1, 7] = np.where(kind[:, K - 1] == M.EMPTY, 0.0, np.maximum(lines[:, K - 1, 7], 10.0))
    targets[:, K - 1] = RR.ANCHOR
    ref, Tref, kinds, SF, ST = RR.wrenches(bodies, lines, targets)
    got, T, state = wrench(rs, bodies, lines, targets)
    assert np.array_equal(state, (kinds == M.TAUT).any(1).astype(np.int32)) and (T >= 0).all()
    some = (state == 1) & ~(along & (kinds == M.TAUT)).any(1)  # a taut line along its arm: its torque cancels (test_moorings_cpu turns them)
    assert some.mean() > 0.5 and (kinds[:, :K - 1] == M.TAUT).mean() > 0.2
    eF = np.abs(got[some, 0:3] - ref[some, 0:3]).max(1) / np.maximum(SF[some], 1e-30)
    eT = np.abs(got[some, 4:7] - ref[some, 4:7]).max(1) / np.maximum(ST[some], 1e-30)
    print("rigged wrench against float64: worst error %.3e of S_F, %.3e of S_tau" % (eF.max(), eT.max()))
    assert eF.max() <= TOL_F and eT.max() <= TOL_TAU, (eF.max(), eT.max())
    assert (got[state == 0] == 0).all()


def tow_shim_run(mw, rs, ps):
    """rig_ref.tow_scene through the shims (the periodic shim's rows on an exactly flat 64^2 mesh, rig_shim's substep) and through
    float64 -> (shim state, float64 state, shim tensions, the scene)"""
    scene = RR.tow_scene(mw)
    hull, tris, _, bodies, mass, wr, lines, targets = scene
    R, uw = 64, 1.0
    rc = S.rest_coords(R, uw).astype(np.float64)
    X, Z = np.meshgrid(rc, rc, indexing="ij")
    vert = np.stack([X, np.zeros_like(X), Z], -1).reshape(-1, 3).astype(np.float32)
    cf = np.array([RR.TOW_RHO, RR.TOW_G, 0.0, 0.0, 1.0], np.float32)
    h = float(np.float32(RR.TOW_DT) / np.float32(RR.TOW_SUB))
    b = bodies.copy()
    for _ in range(RR.TOW_CALLS * RR.TOW_SUB):
        _, rows = PR.hull_forces(ps, R, uw, PR.period(R, uw), vert, None, hull, tris, b, cf)
        T, state = step(rs, b, rows, mass, lines, targets, RR.TOW_G, h, wr)
        assert (state >= 0).all() and (state != 2).all()
    ref, _ = RR.tow_float64(scene)
    return b, ref, T, scene


def test_tow_on_flat_water_against_float64(mw, rs, ps):
    got, ref, T, scene = tow_shim_run(mw, rs, ps)
    start = scene[3]
    err = RR.block_errors(got, ref, start)
    print("tow on flat water, shim against float64, error of the change over the run: " + ", ".join("%s %.3e" % kv for kv in err.items()))
    # the barges follow the tug and both lines pull
    assert (ref[:, 10] > 0.1).all() and (got[:, 10] > 0.1).all() and ref[0, 2] - start[0, 2] > 0.5
    assert T[0, 1] > 0 and T[1, 0] > 0 and T[1, 1] > 0 and T[2, 0] > 0
    # The state's change is the integral of the rows, and a float32 water row is good to 1e-4 of its per-triangle magnitudes
    # (test_hull_sizes_cpu.TOL): the pitching torque is what is left of the hull's pressure moments, about 40 times larger, after they
    # cancel.  So 1e-4 of each block's change bounds the error; a wrong term in the tow slot moves the state by far more.
    assert all(e <= 1e-4 for e in err.values()), err


# ---- 5. validity -------------------------------------------------------------------------------------------------------------------
def test_invalid_bodies_are_held_alone(mw, rs):
    rng = np.random.default_rng(340)
    bodies, mass, rows, wr, lines, targets = _chain_scene(mw, rng, 6)
    n = len(bodies)
    clean = bodies.copy()
    Tc, sc = step(rs, clean, rows, mass, lines, targets, 9.81, 0.02, wr)
    assert (sc == 1).all()

    def run(b0=bodies, ln=lines, tg=targets):
        b = b0.copy()
        T, state = step(rs, b, rows, mass, ln, tg, 9.81, 0.02, wr)
        return b, T, state
    j = 2
    for value in (n, -2, j, 1 << 30, -(1 << 31)):  # out of range either way, and the body itself
        tg = targets.copy()
        tg[j, 1] = value
        b, T, state = run(tg=tg)
        assert state[j] == -1 and np.isnan(T[j]).all() and np.array_equal(_bits(b[j]), _bits(bodies[j])), value
        others = np.arange(n) != j
        assert np.array_equal(_bits(b[others]), _bits(clean[others])) and np.array_equal(_bits(T[others]), _bits(Tc[others]))
        Mo, Tw, sw = wrench(rs, bodies, lines, tg)
        assert sw[j] == -1 and np.isnan(Mo[j]).all() and np.isnan(Tw[j]).all() and (sw[others] == 1).all()
    # the target of an empty slot is not read
    ln, tg = lines.copy(), targets.copy()
    ln[j, 2, 7:9] = 0.0
    tg[j, 2] = 1 << 30
    b, T, state = run(ln=ln, tg=tg)
    assert state[j] == 1 and T[j, 2] == 0 and np.isfinite(b).all()
    # an invalid slot, anchored or towing
    for slot, k, value in ((1, 0, np.nan), (2, 3, -1.0), (0, 7, np.inf)):
        ln = lines.copy()
        ln[j, slot, k] = value
        ln[j, slot, 9:12] = np.nan  # the padding is not read
        b, T, state = run(ln=ln)
        others = np.arange(n) != j
        assert state[j] == -1 and np.isnan(T[j]).all() and np.array_equal(_bits(b[j]), _bits(bodies[j]))
        assert np.array_equal(_bits(b[others]), _bits(clean[others]))
    # a non-finite partner: the bodies tied to it hold with NaN tensions (MW_RIG_LOST), the others are the clean run's
    for k, value in ((0, np.nan), (5, np.inf), (9, -np.inf), (14, np.nan)):
        nb = bodies.copy()
        nb[j, k] = value
        b, T, state = run(b0=nb)
        for tied in (j - 1, j + 1):
            assert state[tied] == 2 and np.isnan(T[tied]).all() and np.array_equal(_bits(b[tied]), _bits(bodies[tied]))
        free = np.array([0, 4, 5])
        assert np.array_equal(_bits(b[free]), _bits(clean[free])) and np.array_equal(_bits(T[free]), _bits(Tc[free]))
    # the padding floats of a partner's state are not read
    nb = bodies.copy()
    nb[j, [3, 11, 15]] = np.nan
    b, T, state = run(b0=nb)
    assert (state == 1).all() and np.array_equal(_bits(b[[1, 3]]), _bits(clean[[1, 3]]))


# ---- 6. exported, declared, bound --------------------------------------------------------------------------------------------------
def test_entry_points_exported_and_bound(mw):
    from mistral_water import _native
    L = mw.lib()
    hdr = open(os.path.join(REPO, "include", "mistral_water.h")).read()
    cs = open(os.path.join(REPO, "bindings", "csharp", "MistralWaterNative.cs")).read()
    for s in ("mw_ocean_step_rigged", "mw_ocean_step_rigged_device"):
        assert hasattr(L, s) and s in _native.ABI_SYMBOLS and s + "(" in hdr and s + "(" in cs
    assert int(re.search(r"#define\s+MW_RIG_ANCHOR\s+\((-?\d+)\)", hdr).group(1)) == _native.MW_RIG_ANCHOR == mw.MW_RIG_ANCHOR == RR.ANCHOR == -1
    assert int(re.search(r"RigAnchor\s*=\s*(-?\d+)", cs).group(1)) == -1
    assert L.mw_abi_version() == 4
    assert hasattr(mw.Ocean, "step_rigged") and hasattr(mw.Ocean, "step_rigged_device")
    assert "no mooring lines yet" not in hdr and "there are no body-to-body lines" not in hdr


def test_step_rigged_bad_arguments_are_statuses(mw):
    L = mw.lib()
    x, t = H.box(1.0, 1.0, 1.0)
    bodies = mw.pack_bodies([[0.0, 0.0, 0.0]])
    before = bodies.copy()
    mass = mw.pack_mass(500.0, np.eye(3) * 80.0)
    lines = mw.pack_lines(1, 1, anchor=[[[0.0, -5.0, 0.0]]], rest_length=1.0, stiffness=10.0)
    table = np.array([[0, 8, 0, 12, 1]], np.int32)
    cf = np.array([1000.0, 9.81, 0, 0, 1], np.float32)
    for fn in (L.mw_ocean_step_rigged, L.mw_ocean_step_rigged_device):
        for K in (1, 0, 9):  # a NULL handle whatever else holds
            assert fn(None, -1, _p(x), 8, _p(t), 12, _p(table), 1, _p(bodies), _p(mass), None, _p(lines), None, K, 1, _p(cf), C.c_float(0.1),
                      1, 0, None, None) == mw.MW_EINVAL
    assert np.array_equal(bodies, before)


def test_the_kernel_uses_the_hd_functions():
    """k_rigged_integrate sums with rig_add and integrates through rig_push; it reads bodies from snap only and writes them to next only;
    rigging.h reuses the moorings' slot, sum and the fleet's pushed row; nothing between workgroups"""
    csrc = os.path.join(REPO, "mistral-water_amd", "csrc")
    src = open(os.path.join(csrc, "rigging.h")).read()
    kern = re.sub(r"//[^\n]*", "", src[src.index("void k_rigged_integrate"):])
    assert "rig_add(&r, body, R, slot, kind, other)" in kern and "rig_push(body, row, mass" in kern and "fleet_map(a.t, MW_FLEET_BODIES" in kern
    assert "a.snap[" not in kern.replace("keep[k] = a.snap[", "") and "a.next[4 * (size_t)b + k] =" in kern and "a.snap +" in kern
    code = re.sub(r"//[^\n]*", "", src)
    for name in ("mooring_add(", "mooring_take(", "mooring_slot_valid(", "fleet_pushed_row(", "fleet_integrate(", "hull_rotation("):
        assert name in code, name
    assert "atomic" not in code and "__threadfence" not in code and "volatile" not in code and "cooperative" not in code
    assert "fp contract(off)" in open(os.path.join(csrc, "moorings.h")).read() and "MW_MOORING_STRICT" in code
