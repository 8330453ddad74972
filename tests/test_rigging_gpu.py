"""GPU tier of the rigged fleets (mw_ocean_step_rigged / _device, include/mistral_water.h) through the C ABI, on small oceans: FFTMesh
64^2 and OceanRenderer resolution 8.  The fleets hold three hull shapes: hull_ref.box (12 triangles), icosphere(subdiv=1) with no
bodies, and icosphere(subdiv=3) (1280 triangles, 5 chunks).

1. states, out and tension after 8 substeps equal, bit for bit, the chain of tests/rig_shim.cpp's substep fed the device's own rows
   (mw_ocean_fleet_forces_device at every intermediate state): 1, 255, 256, 257 and 513 bodies, K = 1 and 8, slots mixed empty, anchored
   and tow (body b tows to b - 1 and to (b + 256) mod n), a periodic, a footprint and an OceanRenderer handle, wrench given and NULL;
2. anchors only (targets NULL and all -1): every body has mw_ocean_step_moored_device's bits on its hull alone;
3. no line taut (all empty; all slack): mw_ocean_step_fleet_device's bits on a periodic handle, test_moorings_gpu.FOOT's bounds on the
   footprint relative to each block's change over the call (an icosphere's w without a wrench does not change -- pressure puts no
   torque on a sphere -- and is held to the same bound relative to |w|);
4. Newton's third law to the bit on a mirrored pair, alone and as 257 interleaved pairs;
5. hull order and body order permuted, targets remapped: every body keeps its bits;
6. a tug towing two barges on flat water against float64 (rig_ref.tow_scene), held to 4x the CPU shim's error on the same scene;
7. a bad target, a self target, an invalid slot and a partner with a NaN pose stay local, between guard words;
8. the argument and state rules, the host form against the device form, the handle's state untouched.

Measured on an MI355X (test 6 prints both): the tow's error relative to each block's change over the run is p 2.525e-7, q 4.593e-6,
v 4.108e-7, w 2.259e-5 on the device and the same figures in tests/rig_shim.cpp."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

import hull_ref as H
import rig_ref as RR
import test_moorings_gpu as TM
import test_rigging_cpu as RC
import workloads  # noqa: F401
from test_moorings_gpu import FOOT, _bits, _ocean, _renderer, _same, _up
from test_rigging_cpu import ps, rs  # noqa: F401  (the shims, as fixtures)

pytestmark = pytest.mark.gpu
RHO = 1000.0
GRAV = (9.81, 9.81, 9.6)  # per hull: the icosphere's bodies fall under another gravity, so that g is read from the body's hull row
EMPTY, ANCHOR_TAUT, ANCHOR_SLACK, TOW_TAUT, TOW_SLACK = range(5)
JUNK = 0x7FFFFFFF  # the target of an empty slot: not read
GUARD = 4096       # guard floats around bodies, out and tension


def _shapes(mw, scale=1.0):
    """[(hull about its centre of mass, triangles, mass row)] of the three shapes at 600 kg/m^3"""
    out = []
    for x, t in (H.box(1.5, 1.0, 2.0), H.icosphere(1.2, 1), H.icosphere(1.2, 3)):
        x = np.asarray(x, np.float64) * scale
        m, c, I = mw.hull_mass_properties(x, t, 600.0)
        out.append((np.asarray(x - c, np.float32), t, mw.pack_mass(m, I)))
    return out


def _coeffs(o, order=(0, 1, 2), gravity=GRAV):
    return np.stack([o._hull_coeffs(RHO, gravity[h], 0.0, 0.0, None) for h in order])


def _fleet(mw, o, rng, n, K, span, scale=1.0, allowed=None, flat_y=None):
    """n bodies -- max(1, n // 6) big icospheres behind the boxes, the small icosphere without bodies -- near the water within +-span,
    and their K slots: slot 0 anchored and taut, slot 1 a tow line to body b - 1, slot 2 one to (b + 256) mod n, the others drawn from
    `allowed` (K = 1: the one slot drawn from all five kinds).  n == 1 has no tow slots.  Taut lines start 0.1 to 0.5 stretched."""
    shapes = _shapes(mw, scale)
    nico = max(1, n // 6)
    counts = [n - nico, 0, nico]
    x, t, table = mw.pack_fleet([(s[0], s[1], c) for s, c in zip(shapes, counts)])
    hull_of = np.repeat([0, 1, 2], counts)
    mass = np.concatenate([np.repeat(s[2], c, 0) for s, c in zip(shapes, counts)])
    pos = np.stack([rng.uniform(-span, span, n), np.zeros(n), rng.uniform(-span, span, n)], 1).astype(np.float32)
    if flat_y is None:
        pos[:, 1] = o.query_surface(np.ascontiguousarray(pos[:, [0, 2]]), mode="world")[:, 1]
        pos[:, 1] += rng.uniform(-0.3, 0.3, n) * scale
    else:
        pos[:, 1] = flat_y
    bodies = mw.pack_bodies(pos, H.upright_quaternions(n, rng, 25.0), rng.standard_normal((n, 3)) * 0.5, rng.standard_normal((n, 3)) * 0.3)
    allowed = list(range(5)) if allowed is None else list(allowed)
    kind = rng.choice(allowed, (n, K))
    if K >= 3 and set(allowed) == set(range(5)):
        kind[:, 0], kind[:, 1], kind[:, 2] = ANCHOR_TAUT, TOW_TAUT, TOW_TAUT
    tow = (kind == TOW_TAUT) | (kind == TOW_SLACK)
    if n == 1:
        kind = np.where(tow, ANCHOR_TAUT, kind)
        tow[:] = False
    b = np.arange(n)
    partner = np.where((np.arange(K) % 2 == 1)[None, :], (b[:, None] - 1) % n, (b[:, None] + 256) % n)
    partner = np.where(partner == b[:, None], (b[:, None] + 1) % n, partner)  # n == 256: (b + 256) mod n is b itself
    targets = np.where(tow, partner, np.where(kind == EMPTY, JUNK, RR.ANCHOR)).astype(np.int32)
    m = mass[:, 0][:, None]
    att = rng.uniform(-0.3, 0.3, (n, K, 3)) * scale
    u = rng.standard_normal((n, K, 3))
    u[:, :, 1] = -np.abs(u[:, :, 1])
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    anchor = pos[:, None, :].astype(np.float64) + u * rng.uniform(3.0, 6.0, (n, K))[:, :, None]
    far = rng.uniform(-0.3, 0.3, (n, K, 3)) * scale
    lines = mw.pack_lines(n, K, attach=att, anchor=np.where(tow[:, :, None], far, anchor),
                          stiffness=np.where(kind == EMPTY, 0.0, rng.uniform(2.0, 6.0, (n, K)) * m),
                          damping=np.where(kind == EMPTY, 0.0, rng.uniform(0.0, 1.0, (n, K)) * m))
    # the length of every line at the start (float64, rig_ref's geometry with L0 = 0, k = 1: T = l), then L0 from it
    probe = lines.copy()
    probe[:, :, 3], probe[:, :, 7], probe[:, :, 8] = 0.0, 1.0, 0.0
    l = RR.slots(bodies, probe, np.where(tow, targets, RR.ANCHOR))[3]
    taut = ((kind == ANCHOR_TAUT) | (kind == TOW_TAUT)) & (l > 1.0)
    lines[:, :, 3] = np.where(taut, l - rng.uniform(0.1, 0.5, (n, K)), 1.5 * l + 1.0)
    wrench = np.zeros((n, 8), np.float32)
    wrench[:, 0:3] = rng.standard_normal((n, 3)) * mass[:, 0:1]
    wrench[:, 4:7] = rng.standard_normal((n, 3)) * mass[:, 1:2] * 0.3
    return SimpleNamespace(x=x, t=t, table=table, hull_of=hull_of, bodies=bodies, mass=mass, lines=lines, targets=targets, wrench=wrench,
                           order=(0, 1, 2), g=np.asarray(GRAV, np.float32)[hull_of], kind=kind, taut=taut, n=n, K=K, shapes=shapes)


def _rigged_device(o, s, dt, substeps, wrench=None, targets="own", bodies=None, lines=None, guard=False):
    """the device form on fresh uploads -> (bodies, out, tension); guard: the three arrays stand between guard words, checked after"""
    import torch
    targets = s.targets if isinstance(targets, str) else targets
    n, K = s.n, s.K
    d_x, d_t, d_m, d_l = _up(s.x, s.t, s.mass, s.lines if lines is None else lines)
    d_w = None if wrench is None else _up(wrench)[0]
    d_g = None if targets is None else _up(np.ascontiguousarray(targets, np.int32))[0]
    sizes = (16 * n, 8 * n, K * n)
    buf = torch.full((sum(sizes) + 4 * GUARD,), 7.0, dtype=torch.float32, device="cuda")
    offs = [GUARD, 2 * GUARD + sizes[0], 3 * GUARD + sizes[0] + sizes[1]]
    view = [buf[a:a + k] for a, k in zip(offs, sizes)]
    view[0].copy_(torch.from_numpy(np.ascontiguousarray(s.bodies if bodies is None else bodies).ravel()))
    torch.cuda.synchronize()
    o.step_rigged_device(d_x.data_ptr(), len(s.x), d_t.data_ptr(), len(s.t), s.table, view[0].data_ptr(), d_m.data_ptr(), d_l.data_ptr(), K, n,
                         dt, substeps, d_targets=0 if d_g is None else d_g.data_ptr(), d_wrench=0 if d_w is None else d_w.data_ptr(),
                         d_out=view[1].data_ptr(), d_tension=view[2].data_ptr(), coeffs=_coeffs(o, s.order))
    o.synchronize()
    host = buf.cpu().numpy()
    if guard:
        keep = np.ones(len(host), bool)
        for a, k in zip(offs, sizes):
            keep[a:a + k] = False
        assert (host[keep] == 7.0).all(), "a guard word around bodies, out or tension was written"
    return tuple(host[a:a + k].reshape(n, -1).copy() for a, k in zip(offs, sizes))


def _rigged_host(o, s, dt, substeps, wrench=None, targets="own"):
    targets = s.targets if isinstance(targets, str) else targets
    return o.step_rigged(s.x, s.t, s.table, s.bodies.copy(), s.mass, s.lines, dt, substeps=substeps, targets=targets, wrench=wrench,
                         coeffs=_coeffs(o, s.order), return_forces=True, return_tension=True)


def _fleet_rows(o, s, bodies):
    import torch
    d_x, d_t, d_b = _up(s.x, s.t, bodies)
    d_o = torch.zeros((len(bodies), 8), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    o.fleet_forces_device(d_x.data_ptr(), len(s.x), d_t.data_ptr(), len(s.t), s.table, d_b.data_ptr(), len(bodies), d_o.data_ptr(),
                          coeffs=_coeffs(o, s.order))
    o.synchronize()
    return d_o.cpu().numpy()


def _chain(rs, o, s, dt, substeps, wrench=None, targets="own", bodies=None, lines=None):  # noqa: F811
    """the shim's substep chain fed the device's own rows -> (state, the last water rows with NaN for the held, the last tensions)"""
    targets = s.targets if isinstance(targets, str) else targets
    h = float(np.float32(dt) / np.float32(substeps))
    b = (s.bodies if bodies is None else bodies).copy()
    for _ in range(substeps):
        rows = _fleet_rows(o, s, b)
        T, state = RC.step(rs, b, rows, s.mass, s.lines if lines is None else lines, targets, s.g, h, wrench)
        rows[(state == -1) | ((state == 2) & ~np.isnan(rows).any(1))] = np.nan  # a NaN water row goes out as the kernels made it
    return b, rows, T


def _compare(got, want, n, tag):
    for g, w, what in zip(got, want, ("state", "out", "tension")):
        bad = np.nonzero((_bits(g) != _bits(w)).reshape(n, -1).any(1))[0]
        assert len(bad) == 0, (what, tag, bad[:5], g[bad[:2]], w[bad[:2]])


# ---- 1. bit for bit against the shim ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 8])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 513])
def test_device_equals_the_shim_bit_for_bit(mw, rs, n, K):  # noqa: F811
    for surface in ("periodic", "footprint", "renderer"):
        rng = np.random.default_rng(100 * n + 10 * K + len(surface))
        o, span, scale = (_renderer(mw), 2.0, 0.3) if surface == "renderer" else (_ocean(mw, periodic=surface == "periodic"),
                                                                                    96.0 if surface == "periodic" else 24.0, 1.0)
        with o:
            s = _fleet(mw, o, rng, n, K, span, scale)
            for wr in (None, s.wrench):
                want = _chain(rs, o, s, 0.16, 8, wr)
                assert np.isfinite(want[0]).all() and np.isfinite(want[1]).all() and not _same(want[0][:, 0:3], s.bodies[:, 0:3])
                if n > 1:
                    tow = (s.kind == TOW_TAUT) & s.taut
                    assert tow.any() and (want[2][tow] > 0).any() and (want[2][s.kind == ANCHOR_TAUT] > 0).any()
                _compare(_rigged_device(o, s, 0.16, 8, wr), want, n, (surface, "device", wr is not None))
                if n in (1, 257):
                    _compare(_rigged_host(o, s, 0.16, 8, wr), want, n, (surface, "host", wr is not None))
            if n == 257:  # an odd count of substeps ends in the caller's array as well, and out is the row of that substep
                _compare(_rigged_device(o, s, 0.06, 3, s.wrench), _chain(rs, o, s, 0.06, 3, s.wrench), n, (surface, "3 substeps"))


# ---- 2. anchors only: step_moored on each hull alone ---------------------------------------------------------------------------------
@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "footprint"])
def test_anchors_only_equals_step_moored(mw, periodic):
    rng = np.random.default_rng(41 + periodic)
    with _ocean(mw, periodic=periodic) as o:
        s = _fleet(mw, o, rng, 70, 8, 96.0 if periodic else 24.0, allowed=(EMPTY, ANCHOR_TAUT, ANCHOR_SLACK))
        assert (s.targets[s.kind != EMPTY] == RR.ANCHOR).all()
        for targets in (None, np.full((s.n, s.K), RR.ANCHOR, np.int32)):
            got = _rigged_device(o, s, 0.16, 8, None, targets)
            for h in (0, 2):
                sl = s.hull_of == h
                hull, tris, _ = s.shapes[h]
                want = TM._moored_device(o, hull, tris, s.bodies[sl], s.mass[sl], s.lines[sl], 0.16, 8, gravity=GRAV[h])
                _compare([g[sl] for g in got], want, int(sl.sum()), (h, targets is None))
                assert (want[2] > 0).any() and np.isfinite(want[0]).all() and not _same(want[0], s.bodies[sl])


# ---- 3. no line taut: step_fleet ----------------------------------------------------------------------------------------------------
def _fleet_device(o, s, dt, substeps, wrench):
    import torch
    d_x, d_t, d_b, d_m = _up(s.x, s.t, s.bodies.copy(), s.mass)
    d_w = None if wrench is None else _up(wrench)[0]
    d_o = torch.full((s.n, 8), 7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    o.step_fleet_device(d_x.data_ptr(), len(s.x), d_t.data_ptr(), len(s.t), s.table, d_b.data_ptr(), d_m.data_ptr(), s.n, dt, substeps,
                        d_wrench=0 if d_w is None else d_w.data_ptr(), d_out=d_o.data_ptr(), coeffs=_coeffs(o, s.order))
    o.synchronize()
    return d_b.cpu().numpy(), d_o.cpu().numpy()


@pytest.mark.parametrize("slots", ["empty", "slack"])
def test_no_line_taut_equals_step_fleet(mw, slots):
    allowed = (EMPTY,) if slots == "empty" else (ANCHOR_SLACK, TOW_SLACK)
    rng = np.random.default_rng(50 + len(slots))
    with _ocean(mw, periodic=True) as o:
        s = _fleet(mw, o, rng, 300, 8, 96.0, allowed=allowed)
        assert slots == "empty" or ((s.targets >= 0).any() and (s.targets == RR.ANCHOR).any())
        for wr in (None, s.wrench):
            got = _rigged_device(o, s, 0.16, 8, wr)
            fb, fo = _fleet_device(o, s, 0.16, 8, wr)
            assert _same(got[0], fb) and _same(got[1], fo) and (got[2] == 0).all() and not _same(fb, s.bodies) and np.isfinite(fb).all()
    with _ocean(mw) as o:  # the footprint: step_fleet integrates with contraction and this call strictly
        s = _fleet(mw, o, rng, 300, 8, 24.0, allowed=allowed)
        for wr in (None, s.wrench):
            got = _rigged_device(o, s, 0.16, 8, wr)
            fb, fo = _fleet_device(o, s, 0.16, 8, wr)
            assert (got[2] == 0).all() and np.isfinite(got[0]).all()
            for key, sl in (("p", slice(0, 3)), ("v", slice(8, 11)), ("w", slice(12, 15)), ("q", slice(4, 8))):
                change = np.linalg.norm(fb[:, sl].astype(np.float64) - s.bodies[:, sl], axis=1)
                if key == "w" and wr is None:
                    # pressure alone puts no torque on a sphere about its centre: without a wrench an icosphere's w changes by
                    # rounding only (1e-5 of |w|), and an error relative to no change says nothing.  Theirs is held to |w| itself.
                    ball = s.hull_of == 2
                    change[ball] = np.linalg.norm(s.bodies[ball, sl], axis=1)
                err = np.abs(got[0][:, sl].astype(np.float64) - fb[:, sl]).max(1)
                assert (err <= FOOT[key] * change).all(), (slots, wr is not None, key, (err / change).max())


# ---- 4. Newton's third law ----------------------------------------------------------------------------------------------------------
def test_a_mirrored_line_pulls_both_ends_alike_to_the_bit(mw):
    x, t = H.box(1.5, 1.0, 2.0)
    m, c, I = mw.hull_mass_properties(x, t, 600.0)
    hull = np.asarray(x - c, np.float32)
    hi, hj, L0 = np.array([0.4, 0.2, -0.3]), np.array([-0.2, 0.1, 0.5]), 5.0
    pair = mw.pack_bodies([[1.3, 50.0, -2.1], [4.9, 52.5, 1.7]], H.upright_quaternions(2, np.random.default_rng(5), 30.0))
    probe, ptg = mw.pack_lines(2, 1), np.zeros((2, 1), np.int32)
    RR.mirror(probe, ptg, 0, 0, 1, 0, hi, hj, 0.0, 1.0)
    l = RR.slots(pair, probe, ptg)[3][0, 0]
    cf = np.array([[RHO, 0.0, 0.0, 0.0, 1.0]], np.float32)  # no gravity: the water rows are zero and nothing falls

    def run(o, npairs):
        n = 2 * npairs
        bodies = np.ascontiguousarray(np.repeat(pair, npairs, 0))  # pair k is bodies k and k + npairs
        lines, targets = mw.pack_lines(n, 1), np.zeros((n, 1), np.int32)
        for k in range(npairs):
            RR.mirror(lines, targets, k, 0, k + npairs, 0, hi, hj, l / 1.2, 8.0 * m, 1.0 * m)  # stretched 20 %
        _, _, table = mw.pack_fleet([(hull, t, n)])
        return o.step_rigged(hull, t, table, bodies, np.repeat(mw.pack_mass(m, I), n, 0), lines, 0.16, substeps=8, targets=targets, coeffs=cf,
                             return_forces=True, return_tension=True)
    with _ocean(mw, periodic=True, flat=True) as o:
        b, rows, T = run(o, 1)
        assert (rows[:, 0:3] == 0).all() and np.isfinite(b).all() and T[0, 0] > 0
        assert np.array_equal(_bits(b[0, 8:11]), _bits(-b[1, 8:11])) and np.array_equal(_bits(T[0]), _bits(T[1]))
        assert np.abs(b[0, 8:11]).max() > 0.1 and not _same(b[:, 0:3], pair[:, 0:3])
        bb, _, TT = run(o, 257)
        assert _same(bb[:257], np.repeat(b[0:1], 257, 0)) and _same(bb[257:], np.repeat(b[1:2], 257, 0))
        assert _same(TT, np.repeat(T, 257, 0))


# ---- 5. order independence ----------------------------------------------------------------------------------------------------------
def test_hull_and_body_order_change_no_bit(mw):
    rng = np.random.default_rng(60)
    with _ocean(mw, periodic=True) as o:
        s = _fleet(mw, o, rng, 257, 8, 96.0)
        want = _rigged_device(o, s, 0.16, 8, s.wrench)
        assert np.isfinite(want[0]).all() and (want[2] > 0).any()
        for order in ((2, 1, 0), (1, 0, 2)):
            new = np.concatenate([rng.permutation(np.nonzero(s.hull_of == h)[0]) for h in order])  # new index -> old index
            inv = np.argsort(new)
            counts = [int((s.hull_of == h).sum()) for h in order]
            x, t, table = mw.pack_fleet([(s.shapes[h][0], s.shapes[h][1], c) for h, c in zip(order, counts)])
            tg = s.targets[new]
            tg = np.where((tg >= 0) & (tg != JUNK), inv[np.clip(tg, 0, s.n - 1)], tg).astype(np.int32)
            p = SimpleNamespace(x=x, t=t, table=table, bodies=np.ascontiguousarray(s.bodies[new]), mass=np.ascontiguousarray(s.mass[new]),
                                lines=np.ascontiguousarray(s.lines[new]), targets=tg, order=order, n=s.n, K=s.K)
            got = _rigged_device(o, p, 0.16, 8, np.ascontiguousarray(s.wrench[new]))
            _compare([g[inv] for g in got], want, s.n, order)


# ---- 6. the tow on flat water against float64 ----------------------------------------------------------------------------------------
def test_tow_on_flat_water_against_float64(mw, rs, ps):  # noqa: F811
    """The device against rig_ref + hull_ref + body_ref in float64 on rig_ref.tow_scene (a tug under a constant wrench, two barges in a
    chain, 16 calls of 8 substeps), each state block relative to its change over the run, held to 4x the error tests/rig_shim.cpp
    shows on the same scene (the factor covers the device's sqrtf and divide rounding paths and nothing else).  No body is left out."""
    shim, ref, _, scene = RC.tow_shim_run(mw, rs, ps)
    hull, tris, table, bodies, mass, wrench, lines, targets = scene
    cf = np.array([[RR.TOW_RHO, RR.TOW_G, 0.0, 0.0, 1.0]], np.float32)
    with _ocean(mw, periodic=True, flat=True) as o:
        b = bodies.copy()
        for _ in range(RR.TOW_CALLS):
            b, rows, T = o.step_rigged(hull, tris, table, b, mass, lines, RR.TOW_DT, substeps=RR.TOW_SUB, targets=targets, wrench=wrench,
                                       coeffs=cf, return_forces=True, return_tension=True)
            assert np.isfinite(rows).all()
    base, err = RR.block_errors(shim, ref, bodies), RR.block_errors(b, ref, bodies)
    for key in base:
        print("tow %s: device %.3e, shim %.3e of the change over the run" % (key, err[key], base[key]))
    assert (b[1:, 10] > 0.1).all() and b[0, 10] > 0.1 and T[0, 1] > 0 and T[1, 1] > 0 and T[1, 0] > 0 and T[2, 0] > 0
    for key in base:
        assert err[key] <= 4 * base[key], (key, err[key], base[key])


# ---- 7. failures stay local ---------------------------------------------------------------------------------------------------------
def _reaches(targets, live, j, hops):
    """the bodies whose state after `hops` substeps can depend on body j: those that reach it along at most `hops` live tow slots"""
    n = len(targets)
    hit = np.zeros(n, bool)
    hit[j] = True
    for _ in range(hops):
        hit = hit | (live & hit[np.clip(targets, 0, n - 1)]).any(1)
    return hit


def test_failures_stay_local(mw, rs):  # noqa: F811
    rng = np.random.default_rng(70)
    n, K, j = 300, 8, 131
    with _ocean(mw, periodic=True) as o:
        s = _fleet(mw, o, rng, n, K, 96.0)
        live = (s.kind == TOW_TAUT) | (s.kind == TOW_SLACK)
        clean = _rigged_device(o, s, 0.16, 8, s.wrench, guard=True)
        assert np.isfinite(clean[0]).all()
        cases = []
        for value in (n, -2, j, 1 << 30):  # a bad target either way, and the body itself
            tg = s.targets.copy()
            tg[j, 1] = value
            cases.append(("target %d" % value, dict(targets=tg), 1))
        for slot, k, value in ((1, 0, np.nan), (0, 3, -1.0), (5, 7, np.inf)):
            ln = s.lines.copy()
            ln[j, slot, k] = value
            ln[j, slot, 9:12] = np.nan
            cases.append(("slot %d float %d" % (slot, k), dict(lines=ln), slot))
        for what, kw, slot in cases:
            got = _rigged_device(o, s, 0.16, 8, s.wrench, guard=True, **kw)
            assert np.isnan(got[1][j]).all() and np.isnan(got[2][j]).all() and _same(got[0][j], s.bodies[j]), what
            _compare(got, _chain(rs, o, s, 0.16, 8, s.wrench, **kw), n, what)
            far = ~_reaches(s.targets, live, j, 8)
            assert far.sum() >= 30 and all(_same(g[far], c[far]) for g, c in zip(got, clean)), what
            with pytest.raises(mw.MistralWaterError) as e:  # the host form names body and slot
                o.step_rigged(s.x, s.t, s.table, s.bodies.copy(), s.mass, kw.get("lines", s.lines), 0.16, substeps=8,
                              targets=kw.get("targets", s.targets), wrench=s.wrench, coeffs=_coeffs(o))
            assert e.value.status == mw.MW_EINVAL and ("slot %d of body %d" % (slot, j)).encode() in mw.lib().mw_last_error(), what
        # a partner with a NaN pose: the bodies with a live tow slot to it hold, with a NaN out row and NaN tensions
        nb = s.bodies.copy()
        nb[j, 0] = np.nan
        got = _rigged_device(o, s, 0.16, 8, s.wrench, bodies=nb, guard=True)
        tied = np.nonzero((live & (s.targets == j)).any(1))[0]
        assert len(tied) >= 2 and j + 1 in tied
        for b in list(tied) + [j]:
            assert np.isnan(got[1][b]).all() and np.isnan(got[2][b]).all() and _same(got[0][b], nb[b]), b
        _compare(got, _chain(rs, o, s, 0.16, 8, s.wrench, bodies=nb), n, "NaN pose")
        far = ~_reaches(s.targets, live, j, 8)
        assert all(_same(g[far], c[far]) for g, c in zip(got, clean))
        near = np.setdiff1d(np.nonzero(~far)[0], np.append(tied, j))
        assert len(near) and np.isfinite(got[0][near]).all() and np.isfinite(got[1][near]).all()  # held neighbours are read as they stand


# ---- 8. arguments and state ---------------------------------------------------------------------------------------------------------
def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def test_argument_checks(mw):
    import torch
    L = mw.lib()
    hull, tris, mrow = TM._hull(mw, "box")
    bodies = mw.pack_bodies([[0.0, 0.0, 0.0], [3.0, 0.0, 0.0]])
    mass = np.repeat(mrow, 2, 0)
    lines = mw.pack_lines(2, 2, anchor=[[[0.0, -5.0, 0.0]] * 2] * 2, rest_length=1.0, stiffness=100.0)
    targets = np.array([[-1, 1], [0, -1]], np.int32)
    table = np.array([[0, 8, 0, 12, 2]], np.int32)
    cf = np.array([RHO, 9.81, 0, 0, 1], np.float32)
    out, ten = np.zeros((2, 8), np.float32), np.zeros((2, 2), np.float32)
    with _ocean(mw) as o:
        h = o._h

        def call(sub=1, dt=0.1, mm=_p(mass), ll=_p(lines), tg=_p(targets), K=2, oo=_p(out), tt=_p(ten), nb=2, frame=-1, ww=None, tb=table):
            return L.mw_ocean_step_rigged(h, frame, _p(hull), 8, _p(tris), 12, _p(tb), 1, _p(bodies), mm, ww, ll, tg, K, nb, _p(cf),
                                          C.c_float(dt), sub, 0, oo, tt)
        none = np.array([[0, 8, 0, 12, 0]], np.int32)
        assert call() == mw.MW_OK and call(oo=None, tt=None, tg=None) == mw.MW_OK
        before = bodies.copy()
        assert call(nb=0, ll=None, tb=none) == mw.MW_OK and _same(bodies, before)  # total_bodies == 0 does nothing
        for kw in (dict(sub=0), dict(sub=65), dict(dt=-0.1), dict(dt=float("nan")), dict(mm=None), dict(frame=0), dict(nb=-1), dict(K=0),
                   dict(K=9), dict(K=-1), dict(ll=None), dict(nb=1)):
            assert call(**kw) == mw.MW_EINVAL, kw
        for bad, where in (([[-1, 2], [0, -1]], b"slot 1 of body 0"), ([[-1, 1], [1, -1]], b"slot 0 of body 1"),
                           ([[-1, 1], [0, -2]], b"slot 1 of body 1")):
            assert call(tg=_p(np.array(bad, np.int32))) == mw.MW_EINVAL and where in L.mw_last_error(), bad
        nan = lines.copy()
        nan[1, 1, 3] = np.nan
        assert call(ll=_p(nan)) == mw.MW_EINVAL and b"slot 1 of body 1" in L.mw_last_error()
        assert _same(bodies, before)
        buf = torch.zeros(64 * 48, dtype=torch.float32, device="cuda")
        base = buf.data_ptr()
        # byte offsets of (bodies, mass, wrench, lines, targets, out, tension) from their aligned places
        for off, want in (((0, 0, 0, 0, 0, 0, 0), mw.MW_OK), ((4, 0, 0, 0, 0, 0, 0), mw.MW_EINVAL), ((0, 8, 0, 0, 0, 0, 0), mw.MW_EINVAL),
                          ((0, 0, 8, 0, 0, 0, 0), mw.MW_EINVAL), ((0, 0, 0, 4, 0, 0, 0), mw.MW_EINVAL), ((0, 0, 0, 8, 0, 0, 0), mw.MW_EINVAL),
                          ((0, 0, 0, 0, 2, 0, 0), mw.MW_EINVAL), ((0, 0, 0, 0, 4, 0, 0), mw.MW_OK), ((0, 0, 0, 0, 0, 4, 0), mw.MW_EINVAL),
                          ((0, 0, 0, 0, 0, 0, 2), mw.MW_EINVAL), ((0, 0, 0, 0, 0, 0, 4), mw.MW_OK)):
            at = [C.c_void_p(base + place + k) for place, k in zip((0, 1024, 8192, 6144, 7168, 2048, 3072), off)]
            st = L.mw_ocean_step_rigged_device(h, -1, C.c_void_p(base + 4096), 8, C.c_void_p(base + 5120), 12, _p(table), 1, at[0], at[1], at[2],
                                               at[3], at[4], 2, 2, _p(cf), C.c_float(0.1), 1, 0, at[5], at[6])
            assert st == want, off
        o.synchronize()
        o.set_column([0.0, 1.0, 3.0])
        o.set_draught(True)  # refused as every fleet entry point
        assert call() == mw.MW_ESTATE and b"draught" in L.mw_last_error() and _same(bodies, before)
        assert L.mw_ocean_step_rigged_device(h, -1, C.c_void_p(base + 4096), 8, C.c_void_p(base + 5120), 12, _p(table), 1, C.c_void_p(base),
                                             C.c_void_p(base + 1024), None, C.c_void_p(base + 6144), None, 2, 2, _p(cf), C.c_float(0.1), 1, 0,
                                             None, None) == mw.MW_ESTATE


def test_step_rigged_changes_no_state(mw):
    """timer, frames, queries and the periodic and column switches are what they are without the rigged calls (the checks of
    test_moorings_gpu.test_step_moored_changes_no_state; draught stays off, where the call is refused)"""
    rng = np.random.default_rng(1)
    xz = np.ascontiguousarray(rng.uniform(-30, 30, (50, 2)), np.float32)
    xyz = np.ascontiguousarray(np.concatenate([xz, rng.uniform(-3, 0, (50, 1)).astype(np.float32)], 1)[:, [0, 2, 1]])
    drag = np.array([[RHO, 9.81, 30.0, 60.0, np.nan]], np.float32)

    def run(with_rigged):
        out = []
        with _ocean(mw, frame=False) as o:
            o.set_column([0.0, 1.0, 2.5])
            for k in range(3):
                v, n, c = o.update(0.03)
                o.set_periodic(k == 1)
                if with_rigged:
                    s = _fleet(mw, None, np.random.default_rng(2), 20, 8, 20.0, flat_y=0.0)
                    _rigged_host(o, s, 0.1, 4, s.wrench)
                    o.step_rigged(s.x, s.t, s.table, s.bodies.copy(), s.mass, s.lines, 0.1, substeps=3, targets=s.targets, coeffs=drag)
                out += [v, n, c, np.float32(o.timer), np.float32(o.periodic), np.float32(o.draught), o.column,
                        o.query_surface(xz, mode="world"), o.query_velocity(xz, mode="world"), o.query_column(xyz)]
        return out

    a, b = run(False), run(True)
    assert len(a) == len(b) and all(_same(np.atleast_1d(x), np.atleast_1d(y)) for x, y in zip(a, b))

    def run_renderer(with_rigged):  # OceanRenderer: the phase, and the frame made from it
        with _renderer(mw) as r:
            if with_rigged:
                s = _fleet(mw, None, np.random.default_rng(3), 12, 8, 2.0, 0.3, flat_y=0.0)
                _rigged_host(r, s, 0.1, 4, s.wrench)
            return [r.get_phase(), *r.generate_texture(0.1), r.get_phase()]

    a, b = run_renderer(False), run_renderer(True)
    assert all(_same(x, y) for x, y in zip(a, b))
