"""numpy float64 reference of the rigged fleets (include/mistral_water.h, csrc/rigging.h), restated independently of the kernels: every
slot of every body at one snapshot of the whole array -- an anchored slot as mooring_ref states it, a tow slot with the anchor replaced by
the target's attachment point x_j = p_j + R(q_j) a and the closing speed (va - vb) . e -- and the rigged substep as body_ref.step under
(water row + wrench) + line wrench.  Rotations are tests/hull_ref.py's."""
import numpy as np

import body_ref as B
import hull_ref as H

ANCHOR = -1
EMPTY, SLACK, TAUT = 0, 1, 2


def _point(bodies, h):
    """(arm d = R(q) h [..., 3], velocity of the point v + w x d) of bodies [..., 16] and body-space points h [..., 3]"""
    R = H.rotation(bodies[..., 4:8].reshape(-1, 4)).reshape(bodies.shape[:-1] + (3, 3))
    d = np.einsum("...ij,...j->...i", R, h)
    return d, bodies[..., 8:11] + np.cross(bodies[..., 12:15], d)


def slots(bodies, lines, targets=None):
    """(kinds [n, K], F [n, K, 3], tau [n, K, 3], T [n, K]) per slot at the snapshot bodies [n, 16]; F, tau and T are 0 unless taut.
    targets [n, K] int (None: all anchored) must be valid for the non-empty slots."""
    b = np.asarray(bodies, np.float64).reshape(-1, 16)
    s = np.asarray(lines, np.float64).reshape(len(b), -1, 12)
    n, K = s.shape[:2]
    t = np.full((n, K), ANCHOR) if targets is None else np.asarray(targets).reshape(n, K)
    L0, k, c = s[:, :, 3], s[:, :, 7], s[:, :, 8]
    empty = (k == 0) & (c == 0)
    tow = ~empty & (t != ANCHOR)
    own = np.broadcast_to(b[:, None, :], (n, K, 16))
    d, va = _point(own, s[:, :, 0:3])
    x = own[:, :, 0:3] + d
    other = b[np.where(tow, t, 0)]  # [n, K, 16]; unused where not tow
    dj, vb = _point(other, s[:, :, 4:7])
    end = np.where(tow[:, :, None], other[:, :, 0:3] + dj, s[:, :, 4:7])
    vb = np.where(tow[:, :, None], vb, 0.0)
    r = end - x
    l = np.linalg.norm(r, axis=2)
    taut = ~empty & (l > L0)
    e = r / np.where(l > 0, l, 1.0)[:, :, None]
    T = np.where(taut, np.maximum(0.0, k * (l - L0) - c * np.einsum("nki,nki->nk", va - vb, e)), 0.0)
    F = T[:, :, None] * e
    return np.where(empty, EMPTY, np.where(taut, TAUT, SLACK)), F, np.cross(d, F), T


def wrenches(bodies, lines, targets=None):
    """(M [n, 8] = (F, 0, tau, 0), tension [n, K], kinds [n, K], S_F [n], S_tau [n]); S_F and S_tau as mooring_ref.wrenches"""
    kinds, F, tau, T = slots(bodies, lines, targets)
    M = np.zeros((len(F), 8))
    M[:, 0:3], M[:, 4:7] = F.sum(1), tau.sum(1)
    return M, T, kinds, np.linalg.norm(F, axis=2).sum(1), np.linalg.norm(tau, axis=2).sum(1)


def step(bodies, rows, mass, lines, targets, g, h, wrench=None):
    """one rigged substep of the whole array bodies [n, 16] under the water rows [n, 8] -> (the new bodies [n, 16] (f64), tension [n, K]);
    g a scalar or [n]; every slot reads the array as it came in"""
    b = np.asarray(bodies, np.float64).reshape(-1, 16)
    M, T = wrenches(b, lines, targets)[:2]
    pushed = np.asarray(rows, np.float64).copy()
    if wrench is not None:
        pushed[:, 0:3] += np.asarray(wrench, np.float64)[:, 0:3]
        pushed[:, 4:7] += np.asarray(wrench, np.float64)[:, 4:7]
    pushed[:, 0:3] += M[:, 0:3]
    pushed[:, 4:7] += M[:, 4:7]
    gs = np.broadcast_to(np.asarray(g, np.float64), (len(b),))
    out = np.stack([B.step(b[i], pushed[i], np.asarray(mass[i], np.float64), float(gs[i]), h) for i in range(len(b))])
    return out, T


def mirror(lines, targets, i, si, j, sj, hi, hj, L0, k, c=0.0):
    """writes the line joining point hi of body i (slot si) and point hj of body j (slot sj) into both bodies' tables, in place"""
    for (a, sa, ha, b, hb) in ((i, si, hi, j, hj), (j, sj, hj, i, hi)):
        lines[a, sa, 0:3], lines[a, sa, 3], lines[a, sa, 4:7], lines[a, sa, 7], lines[a, sa, 8] = ha, L0, hb, k, c
        targets[a, sa] = b


# ---- the tow on flat water (tests/test_rigging_cpu.py test 4, tests/test_rigging_gpu.py test 6) ------------------------------------
TOW_RHO, TOW_G, TOW_DT, TOW_SUB, TOW_CALLS = 1000.0, 9.81, 0.16, 8, 16
BLOCKS = (("p", slice(0, 3)), ("q", slice(4, 8)), ("v", slice(8, 11)), ("w", slice(12, 15)))


def tow_scene(mw):
    """A tug (body 0) under a constant wrench along +z towing two barges in a chain behind it, all the same box floating at its
    equilibrium draught on flat water: (hull, tris, table, bodies [3, 16], mass [3, 8], wrench [3, 8], lines [3, 2, 12], targets [3, 2]).
    The lines run from deck points fore and aft (off the centre of mass, so the boxes pitch), start 5 % stretched, with
    h sqrt(2 k / m) = 0.13 and damping sqrt(k m) along the line; the tug's push would give the three bodies 0.5 m/s^2."""
    x, t = H.box(1.5, 1.0, 2.0)
    m, c, I = mw.hull_mass_properties(x, t, 600.0)
    hull = np.asarray(x - c, np.float32)
    mass = np.repeat(mw.pack_mass(m, I), 3, 0)
    gap = 4.0
    bodies = mw.pack_bodies([[0.3, -0.1, 5.0 - gap * b] for b in range(3)])
    fore, aft = np.array([0.0, 0.3, 0.9]), np.array([0.0, 0.3, -0.9])
    k, L0 = 20.0 * m, (gap - 1.8) / 1.05
    lines, targets = mw.pack_lines(3, 2), np.full((3, 2), ANCHOR, np.int32)
    for b in (0, 1):  # slot 1 of b (aft) to slot 0 of b + 1 (fore)
        mirror(lines, targets, b, 1, b + 1, 0, aft, fore, L0, k, np.sqrt(20.0) * m)
    wrench = np.zeros((3, 8), np.float32)
    wrench[0, 2] = 1.5 * m
    _, _, table = mw.pack_fleet([(hull, t, 3)])
    return hull, t, table, bodies, mass, wrench, lines, targets


def tow_float64(scene):
    """the float64 run of tow_scene: hull_ref.forces on flat water (every vertex resolves: the height is 0), step above -> bodies, T"""
    hull, tris, _, bodies, mass, wrench, lines, targets = scene
    h = float(np.float32(TOW_DT) / np.float32(TOW_SUB))
    ref = bodies.astype(np.float64)
    for _ in range(TOW_CALLS * TOW_SUB):
        x = H.transform(ref, hull)
        rows = np.zeros((len(ref), 8))
        for b in range(len(ref)):
            rows[b, :7] = H.forces(x[b], -x[b, :, 1], np.zeros_like(x[b]), tris, ref[b], TOW_RHO, TOW_G)
        ref, T = step(ref, rows, mass, lines, targets, TOW_G, h, wrench)
    return ref, T


def block_errors(got, ref, start):
    """per state block the worst error over the bodies relative to the block's change over the run: {key: float}"""
    out = {}
    for key, sl in BLOCKS:
        change = np.linalg.norm(np.asarray(ref, np.float64)[:, sl] - np.asarray(start, np.float64)[:, sl], axis=1)
        err = np.abs(np.asarray(got, np.float64)[:, sl] - np.asarray(ref, np.float64)[:, sl]).max(1)
        out[key] = float((err / change).max())
    return out
