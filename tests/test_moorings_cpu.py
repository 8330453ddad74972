"""CPU tier of the moorings (mw_ocean_step_moored / _device, include/mistral_water.h): the model of csrc/moorings.h through
tests/moorings_shim.cpp (g++, strict float32) against tests/mooring_ref.py (numpy float64).

* the mooring wrench of 20 000 random poses for K = 1, 3 and 8 against float64, relative to the sum of the slots' |F| (|tau|);
* the exact properties: no torque from a line through p, nothing from a slack line, body_integrate's bits when every line is slack or
  empty, T >= 0, l == 0, the slot order;
* a surge oscillator and a hanging mass against their closed forms, the angular acceleration of an off-centre line;
* the slot check;
* the new entry points and constants are exported, declared and bound.

Measured (this file's seeds): wrench error 3.61e-6 of S_F and 3.32e-6 of S_tau at worst over the three K (both at K = 1), set by the
float32 positions -- l carries a few ulp(|p|) ~ 1e-6 against a stretch of 0.2 at least -- and not by the sum; the asserted bounds are 8x
those figures rounded up."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import body_ref as B
import hull_ref as H
import mooring_ref as M
import shim_build
from conftest import REPO

SHIM = os.path.join(REPO, "tests", "moorings_shim.cpp")
TOL_F, TOL_TAU = 8 * 3.7e-6, 8 * 3.4e-6  # 8x the measured error of the wrench (test_wrench_against_float64 prints it)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def ms(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("moorings") / "libmoorings_shim.so")
    L = shim_build.strict_f32(SHIM, path)
    L.ms_wrench.restype = None
    L.ms_wrench.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ms_step.restype = None
    L.ms_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
    L.ms_body_integrate.restype = None
    L.ms_body_integrate.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_void_p]
    L.ms_slot_valid.restype = None
    L.ms_slot_valid.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    L.ms_moored_lds_static.restype = C.c_int64
    L.ms_moored_lds_static.argtypes = []
    return L


def wrench(ms, bodies, lines):
    """(M [n, 8], tension [n, K], taut [n]) of the shim"""
    bodies, lines = np.ascontiguousarray(bodies, np.float32), np.ascontiguousarray(lines, np.float32)
    n, K = lines.shape[0], lines.shape[1]
    Mo, T, taut = np.zeros((n, 8), np.float32), np.zeros((n, K), np.float32), np.zeros(n, np.int32)
    ms.ms_wrench(_p(bodies), _p(lines), K, n, _p(Mo), _p(T), _p(taut))
    return Mo, T, taut


def step(ms, bodies, rows, mass, lines, g, h):
    """one moored substep of the shim in place -> (tension [n, K], ok [n])"""
    n, K = lines.shape[0], lines.shape[1]
    T, ok = np.zeros((n, K), np.float32), np.zeros(n, np.int32)
    ms.ms_step(_p(bodies), _p(rows), _p(mass), _p(lines), K, n, g, h, _p(T), _p(ok))
    return T, ok


def random_scene(mw, rng, n, K):
    """n random poses with K slots each: a quarter of the slots empty, of the others half slack (L0 5..50 % above l) and half taut (L0
    20..70 % below l, l in 1..6), so that float32 and float64 agree on which is which and the stretch l - L0 is at least 0.2: the
    positions are float32, so l carries an error of a few ulp(|p|) ~ 1e-6 whatever the arithmetic does, and T inherits it over the stretch.  The damping of a taut slot is drawn relative to its spring
    term: c (va . e) is at most 0.5 k (l - L0) -- the conditioning of T's subtraction is capped at 3, so the measured error is the
    arithmetic's and not how near zero a draw lands -- except about one taut slot in five, sized at 1.1..2 times the spring term: where it
    closes on its anchor it is clamped to T = 0 on both sides."""
    bodies = mw.pack_bodies(rng.standard_normal((n, 3)) * 5, H.random_quaternions(n, rng), rng.standard_normal((n, 3)) * 2,
                            rng.standard_normal((n, 3)))
    lines = mw.pack_lines(n, K)
    lines[:, :, 0:3] = rng.uniform(-1, 1, (n, K, 3))
    d, va, _, _ = M.geometry(bodies, lines)
    u = rng.standard_normal((n, K, 3))
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    # a line nearly along its arm has a torque far below |d| |F| and its cross product cancels: such draws are turned across the arm
    across = np.cross(d, rng.standard_normal((n, K, 3)))
    along = np.linalg.norm(np.cross(d, u), axis=2) < 0.3 * np.linalg.norm(d, axis=2)
    u[along] = (across / np.linalg.norm(across, axis=2, keepdims=True))[along]
    dist = rng.uniform(1.0, 6.0, (n, K))
    lines[:, :, 4:7] = bodies[:, None, 0:3].astype(np.float64) + d + u * dist[:, :, None]
    kind = rng.choice([M.EMPTY, M.SLACK, M.TAUT, M.TAUT], (n, K), p=[0.25, 0.375, 0.1875, 0.1875])
    lines[:, :, 3] = dist * np.where(kind == M.SLACK, rng.uniform(1.05, 1.5, (n, K)), rng.uniform(0.3, 0.8, (n, K)))
    k = rng.uniform(10.0, 1000.0, (n, K))
    _, va, r, l = M.geometry(bodies, lines)  # with the anchors as float32 holds them
    closing = np.abs(np.einsum("nki,nki->nk", va, r / l[:, :, None]))
    # va nearly across the line: the dot product itself cancels, so the damping is sized by 0.2 |va| there and never above the spring
    floor = 0.2 * np.linalg.norm(va, axis=2)
    frac = np.where((rng.uniform(0, 1, (n, K)) < 0.3) & (closing >= floor), rng.uniform(1.1, 2.0, (n, K)), rng.uniform(0.0, 0.5, (n, K)))
    c = frac * k * np.abs(l - lines[:, :, 3]) / np.maximum(closing, floor)
    lines[:, :, 7] = np.where(kind == M.EMPTY, 0.0, k)
    lines[:, :, 8] = np.where(kind == M.EMPTY, 0.0, np.where(kind == M.SLACK, rng.uniform(0, 20, (n, K)), c))
    return bodies, lines


@pytest.mark.parametrize("K", [1, 3, 8])
def test_wrench_against_float64(mw, ms, K):
    rng = np.random.default_rng(100 + K)
    n = 20000
    bodies, lines = random_scene(mw, rng, n, K)
    ref, Tref, kinds, SF, ST = M.wrenches(bodies, lines)
    for kind in (M.EMPTY, M.SLACK, M.TAUT):
        assert (kinds == kind).mean() >= 0.10, kind
    assert ((kinds == M.TAUT) & (Tref == 0)).mean() >= 0.01  # and the clamp is in the mix
    got, T, taut = wrench(ms, bodies, lines)
    assert np.array_equal(taut, (kinds == M.TAUT).any(1).astype(np.int32))
    assert np.array_equal(T > 0, Tref > 0) and (T >= 0).all()
    some = taut == 1
    eF = np.abs(got[some, 0:3] - ref[some, 0:3]).max(1) / np.maximum(SF[some], 1e-30)
    eT = np.abs(got[some, 4:7] - ref[some, 4:7]).max(1) / np.maximum(ST[some], 1e-30)
    clamped_only = SF[some] == 0  # every taut slot of the body clamped: the sum is exactly 0 on both sides
    assert (got[some][clamped_only][:, [0, 1, 2, 4, 5, 6]] == 0).all()
    eF, eT = eF[~clamped_only], eT[~clamped_only & (ST[some] > 0)]
    print(f"K={K}: wrench error {eF.max():.3e} of S_F, {eT.max():.3e} of S_tau; tension "
          f"{(np.abs(T - Tref) / np.maximum(np.abs(Tref), 1e-30))[Tref > 0].max():.3e}")
    assert eF.max() <= TOL_F and eT.max() <= TOL_TAU
    assert (got[~some] == 0).all() and (got[:, [3, 7]] == 0).all()


def _one(mw, p=(0, 0, 0), q=None, v=None, w=None):
    return mw.pack_bodies([p], None if q is None else [q], None if v is None else [v], None if w is None else [w])


def test_line_through_p_has_no_torque(mw, ms):
    rng = np.random.default_rng(1)
    n = 500
    bodies = mw.pack_bodies(rng.standard_normal((n, 3)) * 5, H.random_quaternions(n, rng), rng.standard_normal((n, 3)),
                            rng.standard_normal((n, 3)))
    lines = mw.pack_lines(n, 1, anchor=rng.standard_normal((n, 1, 3)) * 8, rest_length=0.1, stiffness=300.0, damping=2.0)
    got, T, taut = wrench(ms, bodies, lines)
    assert (taut == 1).all() and (T > 0).any()
    assert (got[:, 4:7] == 0).all() and (np.abs(got[:, 0:3]).max(1) > 0).any()


def test_slack_and_empty_slots_contribute_nothing(mw, ms):
    body = _one(mw, (1.0, 2.0, 3.0), v=(0.3, -0.2, 0.1), w=(0.5, 0.4, -0.3))
    taut = mw.pack_lines(1, 1, attach=[[[0.5, 0.2, -0.1]]], anchor=[[[4.0, 2.0, 3.0]]], rest_length=1.0, stiffness=100.0, damping=3.0)
    slack = mw.pack_lines(1, 1, attach=[[[0.1, 0.0, 0.3]]], anchor=[[[1.0, 4.0, 3.0]]], rest_length=5.0, stiffness=1e6, damping=1e3)
    exact = slack.copy()  # l == L0 exactly: still slack
    exact[0, 0, 0:3] = 0
    exact[0, 0, 4:7] = [1.0, 2.0, 7.0]
    exact[0, 0, 3] = 4.0
    empty = mw.pack_lines(1, 1, attach=[[[0.1, 0.0, 0.3]]], anchor=[[[9.0, 4.0, 3.0]]], rest_length=0.5)
    alone, Ta, _ = wrench(ms, body, taut)
    for other in (slack, exact, empty):
        Mo, To, t = wrench(ms, body, other)
        assert t[0] == 0 and (Mo == 0).all() and (To == 0).all()
        for order in ((taut, other), (other, taut), (other, taut, other)):
            both, Tb, t = wrench(ms, body, np.concatenate(order, 1))
            assert t[0] == 1 and np.array_equal(_bits(both), _bits(alone))
            assert sorted(Tb[0]) == sorted([Ta[0, 0]] + [0.0] * (len(order) - 1))


def test_all_slack_leaves_body_integrate_bits(mw, ms):
    """every slot slack or empty: the substep is body_integrate on the bare row, rows holding -0.0 included.  Whether a +0.0 was added to
    a -0.0 entry does not show in a moving body, so a body at rest with v = -0.0 under a -0.0 row and g = 0 is stepped as well: its v stays
    -0.0 only if the row went into the integrator as it was."""
    rng = np.random.default_rng(2)
    n, K = 300, 4
    bodies = mw.pack_bodies(rng.standard_normal((n, 3)) * 3, H.random_quaternions(n, rng), rng.standard_normal((n, 3)), rng.standard_normal((n, 3)))
    masses = rng.uniform(0.5, 50.0, n)
    mass = mw.pack_mass(masses, np.eye(3)[None] * masses[:, None, None])
    rows = (rng.standard_normal((n, 8)) * 10).astype(np.float32)
    rows[::3, 0:3] = -0.0
    rows[1::3, 4:7] = -0.0
    rows[5] = -0.0
    lines = mw.pack_lines(n, K, attach=rng.uniform(-1, 1, (n, K, 3)), anchor=bodies[:, None, 0:3] + rng.uniform(-1, 1, (n, K, 3)),
                          rest_length=50.0, stiffness=500.0, damping=5.0)
    lines[:, 1, 7:9] = 0  # an empty slot among them
    a, b = bodies.copy(), bodies.copy()
    T, ok = step(ms, a, rows, mass, lines, 9.81, 0.01)
    okb = np.zeros(n, np.int32)
    ms.ms_body_integrate(_p(b), _p(rows), _p(mass), n, 9.81, 0.01, _p(okb))
    assert (ok == 1).all() and (okb == 1).all() and (T == 0).all()
    assert np.array_equal(_bits(a), _bits(b)) and not np.array_equal(a, bodies)
    # v = -0.0 + h (-0.0 / m) = -0.0; with a +0.0 added to the row it would be -0.0 + h (+0.0 / m) = +0.0
    still = mw.pack_bodies([[0.0, 0.0, 0.0]])
    still[0, 8:11] = -0.0
    row = np.full((1, 8), -0.0, np.float32)
    step(ms, still, row, mass[:1], lines[:1], 0.0, 0.01)
    assert np.signbit(still[0, 8:11]).all()


def test_tension_is_never_negative(mw, ms):
    """closing on the anchor faster than the spring pulls: c (va . e) > k (l - L0), T = 0 and no push"""
    body = _one(mw, (0.0, 0.0, 0.0), v=(3.0, 0.0, 0.0))
    lines = mw.pack_lines(1, 1, anchor=[[[5.0, 0.0, 0.0]]], rest_length=4.0, stiffness=10.0, damping=20.0)  # 10 * 1 - 20 * 3 < 0
    ref = M.slots(body, lines)
    assert ref[0][0, 0] == M.TAUT and ref[3][0, 0] == 0
    got, T, taut = wrench(ms, body, lines)
    assert T[0, 0] == 0 and not np.signbit(T[0, 0]) and (got[0, [0, 1, 2, 4, 5, 6]] == 0).all()
    lines[0, 0, 8] = 1.0  # 10 - 3 = 7 > 0
    got, T, _ = wrench(ms, body, lines)
    assert T[0, 0] == 7.0 and got[0, 0] == 7.0
    rng = np.random.default_rng(3)
    bodies, many = random_scene(mw, rng, 4000, 8)
    many[:, :, 8] *= 4  # much more damping than the scene draws
    assert (wrench(ms, bodies, many)[1] >= 0).all()


def test_zero_length_is_finite(mw, ms):
    body = _one(mw, (1.0, -2.0, 0.5), v=(1.0, 1.0, 1.0), w=(1.0, 2.0, 3.0))
    for L0 in (0.0, 1.0):
        lines = mw.pack_lines(1, 2, anchor=[[[1.0, -2.0, 0.5]] * 2], rest_length=L0, stiffness=100.0, damping=[[10.0, 0.0]])
        got, T, taut = wrench(ms, body, lines)
        assert taut[0] == 0 and np.isfinite(got).all() and (got == 0).all() and (T == 0).all()


def test_slot_order(mw, ms):
    """the sum runs in slot order from the first taut slot's own value: a by-hand float32 sum of the slots' single-slot wrenches
    reproduces the shim bit for bit, and a permutation of the slots changes at most rounding"""
    rng = np.random.default_rng(4)
    n, K = 2000, 8
    bodies, lines = random_scene(mw, rng, n, K)
    got, T, taut = wrench(ms, bodies, lines)
    hand = np.zeros((n, 8), np.float32)
    begun = np.zeros(n, bool)
    for s in range(K):
        one, T1, t1 = wrench(ms, bodies, lines[:, s:s + 1])
        assert np.array_equal(_bits(T1[:, 0]), _bits(T[:, s]))
        first, later = (t1 == 1) & ~begun, (t1 == 1) & begun
        hand[first] = one[first]
        hand[later] = hand[later] + one[later]  # float32 adds, one per entry
        begun |= t1 == 1
    assert np.array_equal(begun, taut == 1) and np.array_equal(_bits(hand), _bits(got))
    perm = rng.permutation(K)
    other, Tp, _ = wrench(ms, bodies, np.ascontiguousarray(lines[:, perm]))
    assert np.array_equal(_bits(Tp), _bits(T[:, perm]))
    assert not np.array_equal(_bits(other), _bits(got))  # the floats differ, so some sum rounds differently
    _, _, _, SF, ST = M.wrenches(bodies, lines)
    assert (np.abs(other[:, 0:3] - got[:, 0:3]).max(1) <= 2 * TOL_F * SF).all()
    assert (np.abs(other[:, 4:7] - got[:, 4:7]).max(1) <= 2 * TOL_TAU * ST).all()


def test_surge_oscillator(mw, ms):
    """a point-like box between two opposing pre-stretched lines through its centre of mass, no water, g = 0: a spring of 2k while
    neither line goes slack.  h omega = 0.05: the integrator's own period error is (h omega)^2 / 24 ~ 1e-4; 1 % is test_heave_period's
    margin, and the amplitude stays within [0.9, 1.01] of its start as there."""
    m, k, D, L0, x0, h = 100.0, 50.0, 10.0, 5.0, 0.5, 0.05
    omega = np.sqrt(2 * k / m)
    assert h * omega <= 0.1
    Tp = 2 * np.pi / omega
    body = _one(mw, (x0, 0.0, 0.0))
    mass = mw.pack_mass(m, B.box_inertia(m, 0.1, 0.1, 0.1))
    lines = mw.pack_lines(1, 2, anchor=[[[D, 0.0, 0.0], [-D, 0.0, 0.0]]], rest_length=L0, stiffness=k)
    rows = np.zeros((1, 8), np.float32)
    xs, ts = [x0], [0.0]
    while ts[-1] < 3.3 * Tp:
        T, ok = step(ms, body, rows, mass, lines, 0.0, h)
        assert ok[0] == 1 and (T > 0).all()  # neither line slack
        xs.append(float(body[0, 0]))
        ts.append(ts[-1] + h)
    xs, ts = np.array(xs), np.array(ts)
    kk = np.nonzero((xs[:-1] > 0) & (xs[1:] <= 0))[0]  # downward crossings
    tc = ts[kk] + (ts[kk + 1] - ts[kk]) * xs[kk] / (xs[kk] - xs[kk + 1])
    assert len(tc) >= 3
    period = (tc[-1] - tc[0]) / (len(tc) - 1)
    assert abs(period - Tp) <= 0.01 * Tp, (period, Tp)
    assert 0.9 * x0 <= xs.max() <= 1.01 * x0 and -1.01 * x0 <= xs.min() <= -0.9 * x0
    assert (body[0, [1, 2]] == 0).all() and (body[0, 12:15] == 0).all()


def test_hanging_mass(mw, ms):
    """one vertical line, gravity on, critical damping c = 2 sqrt(k m), run for 20 / omega: the transient is e^-20 by then and the
    extension is m g / k to float32 rounding of the position (an ulp of p.y ~ 8 is 5e-6 of the extension; 1e-4 is loose on purpose)"""
    m, k, g, L0, top = 10.0, 1000.0, 9.81, 2.0, 10.0
    omega = np.sqrt(k / m)
    h = 0.005
    assert h * omega <= 0.1
    body = _one(mw, (0.0, top - L0, 0.0))
    mass = mw.pack_mass(m, B.box_inertia(m, 0.2, 0.2, 0.2))
    lines = mw.pack_lines(1, 1, anchor=[[[0.0, top, 0.0]]], rest_length=L0, stiffness=k, damping=2 * np.sqrt(k * m))
    rows = np.zeros((1, 8), np.float32)
    for _ in range(int(np.ceil(20 / omega / h))):
        T, ok = step(ms, body, rows, mass, lines, g, h)
        assert ok[0] == 1
    ext = (top - float(body[0, 1])) - L0
    assert abs(ext - m * g / k) <= 1e-4 * m * g / k, (ext, m * g / k)
    assert abs(float(T[0, 0]) - m * g) <= 1e-4 * m * g and (body[0, [0, 2]] == 0).all()


def test_off_centre_line_angular_acceleration(mw, ms):
    """a body at rest under one off-centre line: w after the first substep is h I_w^-1 tau of mooring_ref, within the wrench tolerance
    (carried through I_w^-1: the bound is TOL_TAU |I_w^-1| S_tau) plus the integrator's own 4e-6 (test_integration_step_against_reference)"""
    rng = np.random.default_rng(6)
    n = 400
    bodies = mw.pack_bodies(rng.standard_normal((n, 3)) * 5, H.random_quaternions(n, rng))
    m = 40.0
    Ib = B.box_inertia(m, 2.0, 1.0, 3.0)
    mass = mw.pack_mass(np.full(n, m), Ib)
    lines = mw.pack_lines(n, 1, attach=rng.uniform(-1, 1, (n, 1, 3)), anchor=bodies[:, None, 0:3] + rng.standard_normal((n, 1, 3)) * 6,
                          rest_length=0.5, stiffness=200.0)
    ref, _, kinds, _, ST = M.wrenches(bodies, lines)
    assert (kinds == M.TAUT).all()
    h = 0.01
    out = bodies.copy()
    step(ms, out, np.zeros((n, 8), np.float32), mass, lines, 0.0, h)
    R = H.rotation(bodies[:, 4:8])
    Iw_inv = np.einsum("nij,jk,nlk->nil", R, np.linalg.inv(np.asarray(Ib, np.float64)), R)
    alpha = np.einsum("nij,nj->ni", Iw_inv, ref[:, 4:7])
    got = out[:, 12:15].astype(np.float64) / h
    bound = (TOL_TAU + 4e-6) * np.linalg.norm(Iw_inv, 2, axis=(1, 2)) * ST
    assert (np.abs(got - alpha).max(1) <= bound).all(), (np.abs(got - alpha).max(1) / bound).max()
    assert (np.linalg.norm(alpha, axis=1) > 100 * bound).mean() > 0.9  # the check has teeth


def test_slot_check(mw, ms):
    good = np.array([0.5, -0.2, 0.1, 2.0, 3.0, 4.0, -5.0, 100.0, 3.0, 0.0, 0.0, 0.0], np.float32)
    rows = [good]
    for k in range(9):
        for bad in (np.nan, np.inf, -np.inf):
            r = good.copy()
            r[k] = bad
            rows.append(r)
    for k in (3, 7, 8):
        r = good.copy()
        r[k] = -1e-3
        rows.append(r)
    nbad = len(rows) - 1
    for k in (9, 10, 11):  # the padding is not read
        for pad in (np.nan, np.inf, -7.0):
            r = good.copy()
            r[k] = pad
            rows.append(r)
    zero = good.copy()
    zero[[3, 7, 8]] = [0.0, -0.0, 0.0]  # zeros of either sign are not negative
    rows.append(zero)
    rows = np.ascontiguousarray(rows, np.float32)
    ok = np.zeros(len(rows), np.int32)
    ms.ms_slot_valid(_p(rows), len(rows), _p(ok))
    assert list(ok) == [1] + [0] * nbad + [1] * (len(rows) - 1 - nbad)
    # through the wrench and the step: NaN wrench and tensions, the body untouched; an invalid slot counts even when it is empty
    body = _one(mw, (0.0, 1.0, 0.0), v=(1.0, 0.0, 0.0))
    lines = np.stack([good, rows[1]])[None]
    lines[0, 1, 7:9] = 0
    Mo, T, taut = wrench(ms, body, lines)
    assert taut[0] == -1 and np.isnan(Mo).all() and np.isnan(T).all()
    b = body.copy()
    T, okk = step(ms, b, np.zeros((1, 8), np.float32), mw.pack_mass(1.0, np.eye(3)), np.ascontiguousarray(lines), 9.81, 0.01)
    assert okk[0] == -1 and np.isnan(T).all() and np.array_equal(_bits(b), _bits(body))


def test_pack_lines(mw):
    ln = mw.pack_lines(3, 2)
    assert ln.shape == (3, 2, 12) and ln.dtype == np.float32 and (ln == 0).all()
    ln = mw.pack_lines(2, 3, attach=[0.1, 0.2, 0.3], anchor=np.arange(18).reshape(2, 3, 3), rest_length=[1.0, 2.0, 3.0], stiffness=50.0,
                       damping=[[1.0], [2.0]])
    assert (ln[:, :, 0:3] == np.float32([0.1, 0.2, 0.3])).all() and (ln[1, 2, 4:7] == [15, 16, 17]).all()
    assert (ln[:, :, 3] == [1.0, 2.0, 3.0]).all() and (ln[:, :, 7] == 50.0).all() and (ln[1, :, 8] == 2.0).all() and (ln[:, :, 9:] == 0).all()
    for K in (0, 9):
        with pytest.raises(ValueError):
            mw.pack_lines(1, K)


def test_entry_points_exported_and_bound(mw):
    from mistral_water import _native
    L = mw.lib()
    hdr = open(os.path.join(REPO, "include", "mistral_water.h")).read()
    for s in ("mw_ocean_step_moored", "mw_ocean_step_moored_device"):
        assert hasattr(L, s) and s in _native.ABI_SYMBOLS and s + "(" in hdr
    cs = open(os.path.join(REPO, "bindings", "csharp", "MistralWaterNative.cs")).read()
    for name, cname, value in (("MW_MOORING_MAX_LINES", "MooringMaxLines", 8), ("MW_MOORING_NLINE", "MooringNLine", 12)):
        assert int(re.search(r"#define\s+" + name + r"\s+(\d+)", hdr).group(1)) == getattr(_native, name) == getattr(mw, name) == value
        assert int(re.search(cname + r"\s*=\s*(\d+)", cs).group(1)) == value
    assert L.mw_abi_version() == 4
    assert hasattr(mw.Ocean, "step_moored") and hasattr(mw.Ocean, "step_moored_device")


def test_step_moored_bad_arguments_are_statuses(mw):
    L = mw.lib()
    x, t = H.box(1.0, 1.0, 1.0)
    bodies = mw.pack_bodies([[0.0, 0.0, 0.0]])
    mass = mw.pack_mass(500.0, B.box_inertia(500.0, 1, 1, 1))
    lines = mw.pack_lines(1, 1, anchor=[[[0.0, -5.0, 0.0]]], rest_length=1.0, stiffness=10.0)
    cf = np.array([1000.0, 9.81, 0, 0, 1], np.float32)
    before = bodies.copy()
    for fn in (L.mw_ocean_step_moored, L.mw_ocean_step_moored_device):
        for K in (1, 0, 9):
            assert fn(None, -1, _p(x), 8, _p(t), 12, _p(bodies), _p(mass), _p(lines), K, 1, _p(cf), C.c_float(0.1), 1, 0, None,
                      None) == mw.MW_EINVAL
    assert np.array_equal(bodies, before)


def test_kernels_use_the_hd_functions():
    """both plans compute the wrench with mooring_add / mooring_wrench and integrate through fleet_integrate; the one-launch kernel is
    the strict k_fleet_step (k_bodies_step's loop, the shared ordered sums); the rigged fleets' own-slot branch is mooring_add; nothing
    between workgroups"""
    csrc = os.path.join(REPO, "mistral-water_amd", "csrc")
    src = open(os.path.join(csrc, "moorings.h")).read()
    integ = src[src.index("void k_moored_integrate"):]
    assert "mooring_add(&m, body, R, slot)" in integ and "fleet_integrate(body, row, mass, m.any ? m.M : nullptr, a.g, a.dt)" in integ
    fleet = open(os.path.join(csrc, "fleet.h")).read()
    stepk = fleet[fleet.index("void k_fleet_step"):]
    assert "moored_integrate(body, pushed, mass, slots, K, it.row.g, a.dt, tens)" in stepk
    assert "fleet_pushed_row(row, a.wrench ? wr : nullptr, pushed)" in stepk
    moored = src[src.index("MW_HD bool moored_integrate("):src.index("#define MW_MOORED_LDS_STATIC")]
    assert "mooring_wrench(body, lines, K, M, tension)" in moored
    assert "fleet_integrate(body, row, mass, taut > 0 ? M : nullptr, g, h)" in moored
    assert "hull_vertex(a.m, vel, it.row.vscale, a.iters, body, h, sl)" in stepk and "hull_row(acc, res, row)" in stepk
    assert "hull_triangle(idx, nverts, vs, body, it.row.cf, acc)" in stepk
    assert "hull_chunk_partial(acc, res, part + 2 * c)" in stepk and "hull_body_sum(part, 0, " in stepk
    services = open(os.path.join(csrc, "surface_services.inc")).read()
    launch = services[services.index("static mw_status moored_launch("):services.index("// ---- the hull family's entry points")]
    assert "strict_moored_integrate(gi, o->stream, a)" in launch and "hull_step_launch(o, p, c)" in launch
    rig = open(os.path.join(csrc, "rigging.h")).read()
    add = rig[rig.index("MW_HD float rig_add("):rig.index("// what rig_wrench and rigged_integrate report")]
    assert "if (kind != MW_RIG_SLOT_TOW) {" in add and "return mooring_add(&r->m, body, R, s);" in add
    rigk = rig[rig.index("void k_rigged_integrate"):]
    assert "rig_add(&r, body, R, slot, kind, other)" in rigk and "rig_push(body, row, mass" in rigk
    bodies = open(os.path.join(csrc, "rigid_bodies.h")).read()
    assert "moor" not in bodies  # k_bodies_step took no parameter for this
    code = re.sub(r"//[^\n]*", "", src)
    assert "atomic" not in code and "__threadfence" not in code and "volatile" not in code and "__shfl" not in code
    assert "fp contract(off)" in src
