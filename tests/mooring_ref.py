"""numpy float64 reference of the moorings (include/mistral_water.h, csrc/moorings.h), restated independently of the kernels: the line
force as the header's six steps state it, with x - p taken literally, over all bodies and slots at once, and the moored substep as
body_ref.step under the water row plus the mooring wrench.  Rotations are tests/hull_ref.py's.  Below it, the helpers of the size tests
(tests/test_mooring_sizes_cpu.py, tests/test_mooring_sizes_gpu.py): the device-free float32 reference chain, the lines of a scene and the
conditions a scene has to meet."""
import numpy as np

import body_ref as B
import hull_ref as H

EMPTY, SLACK, TAUT = 0, 1, 2


def geometry(bodies, lines):
    """(x - p [n, K, 3], va [n, K, 3], r [n, K, 3], l [n, K]) of bodies [n, 16] under lines [n, K, 12]: steps 1-3"""
    b = np.asarray(bodies, np.float64).reshape(-1, 16)
    s = np.asarray(lines, np.float64).reshape(len(b), -1, 12)
    p = b[:, None, 0:3]
    x = p + np.einsum("nij,nkj->nki", H.rotation(b[:, 4:8]), s[:, :, 0:3])
    va = b[:, None, 8:11] + np.cross(b[:, None, 12:15], x - p)
    r = s[:, :, 4:7] - x
    return x - p, va, r, np.linalg.norm(r, axis=2)


def slots(bodies, lines):
    """(kinds [n, K], F [n, K, 3], tau [n, K, 3], T [n, K]) per slot; F, tau and T are 0 unless the line is taut"""
    s = np.asarray(lines, np.float64)
    s = s.reshape(-1, s.shape[-2], 12)
    d, va, r, l = geometry(bodies, s)
    L0, k, c = s[:, :, 3], s[:, :, 7], s[:, :, 8]
    empty = (k == 0) & (c == 0)
    taut = ~empty & (l > L0)
    e = r / np.where(l > 0, l, 1.0)[:, :, None]
    T = np.where(taut, np.maximum(0.0, k * (l - L0) - c * np.einsum("nki,nki->nk", va, e)), 0.0)
    F = T[:, :, None] * e
    kinds = np.where(empty, EMPTY, np.where(taut, TAUT, SLACK))
    return kinds, F, np.cross(d, F), T


def wrenches(bodies, lines):
    """(M [n, 8] = (F, 0, tau, 0), tension [n, K], kinds [n, K], S_F [n], S_tau [n]): S_F and S_tau are the sums over a body's slots of
    |F| and |tau|, the scales a rounding error of the sum is measured against"""
    kinds, F, tau, T = slots(bodies, lines)
    M = np.zeros((len(F), 8))
    M[:, 0:3], M[:, 4:7] = F.sum(1), tau.sum(1)
    return M, T, kinds, np.linalg.norm(F, axis=2).sum(1), np.linalg.norm(tau, axis=2).sum(1)


def step(body, row, mass_row, lines, g, h):
    """one moored substep of body [16] under the water row [8] and lines [K, 12] -> the new body [16] (f64)"""
    M = wrenches(np.asarray(body)[None], np.asarray(lines)[None])[0][0]
    pushed = np.asarray(row, np.float64).copy()
    pushed[0:3] += M[0:3]
    pushed[4:7] += M[4:7]
    return B.step(body, pushed, mass_row, g, h)


# ---- the device-free reference chain (tests/test_mooring_sizes_cpu.py, tests/test_mooring_sizes_gpu.py) -----------------------------
def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def chain(ms, rows_of, bodies, mass, lines, g, dt, substeps, trace=None):
    """The moored call restated without a device value: per substep rows_of(state [n, 16]) -> the water rows [n, 8] of an ordered g++
    shim (periodic_ref.hull_forces, draught_ref.forces), then one substep of tests/moorings_shim.cpp (test_moorings_cpu.step) with
    h = float32(dt) / float32(substeps).  -> (state, the last rows, the tensions at the start of the last substep).  trace: a list that
    receives (state at the start, rows, tensions) of every substep."""
    import test_moorings_cpu as TC
    h = float(np.float32(dt) / np.float32(substeps))
    b = np.array(bodies, np.float32, copy=True)
    mass, lines = np.ascontiguousarray(mass, np.float32), np.ascontiguousarray(lines, np.float32)
    for _ in range(substeps):
        start = b.copy()
        rows = np.ascontiguousarray(rows_of(b), np.float32)
        T, _ = TC.step(ms, b, rows, mass, lines, g, h)
        if trace is not None:
            trace.append((start, rows, T))
    return b, rows, T


def moor(mw, rng, bodies, mass, K, h, period=None, reach=(2.7, 0.6, 2.7)):
    """lines [n, K, 12] for the bodies as test_moorings_gpu._scene draws them, and their kinds [n, K]: slot 0 taut and the others a mix
    of taut, slack and empty; every attachment point within +-reach in body space (inside the edge hulls' 6 x 1.5 x 6 box); every anchor
    3 to 6 from its attachment point, below and beside it, mirrored back when it would leave its body's tile of a sea of that period;
    L0 = 0.8 of that distance (taut) or 1.5 (slack); k = 0.5 .. 0.95 of m (0.2 / h)^2 / 8, so that h sqrt(8 k / m) < 0.2 with all K
    lines along one direction; c up to k / 4 per second, test_moorings_gpu._scene's proportion."""
    b = np.asarray(bodies, np.float64)
    n = len(b)
    m = np.asarray(mass, np.float64)[:, 0][:, None]
    att = rng.uniform(-1.0, 1.0, (n, K, 3)) * np.asarray(reach)
    x = b[:, None, 0:3] + np.einsum("nij,nkj->nki", H.rotation(b[:, 4:8]), att)
    u = rng.standard_normal((n, K, 3))
    u[:, :, 1] = -np.abs(u[:, :, 1])
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    dist = rng.uniform(3.0, 6.0, (n, K))
    kind = rng.choice([EMPTY, SLACK, TAUT], (n, K))
    kind[:, 0] = TAUT
    off = u * dist[:, :, None]
    if period:
        tile = np.floor((b[:, None, [0, 2]] + period / 2) / period)
        leaves = np.floor((x[:, :, [0, 2]] + off[:, :, [0, 2]] + period / 2) / period) != tile
        off[:, :, 0] = np.where(leaves[:, :, 0], -off[:, :, 0], off[:, :, 0])
        off[:, :, 2] = np.where(leaves[:, :, 1], -off[:, :, 2], off[:, :, 2])
    kmax = m * (0.2 / h) ** 2 / 8.0
    k = np.where(kind == EMPTY, 0.0, rng.uniform(0.5, 0.95, (n, K)) * kmax)
    lines = mw.pack_lines(n, K, attach=att, anchor=x + off, rest_length=dist * np.where(kind == SLACK, 1.5, 0.8), stiffness=k,
                          damping=rng.uniform(0.0, 0.25, (n, K)) * k)
    return lines, kind


def scene_is_live(ms, bodies, lines, want, trace, nsentinels, wet_throughout=False):
    """the conditions a scene of edge hulls has to meet for a comparison with want, trace = chain(...) to mean something, on the
    reference alone: every body starts with a taut slot; at least half of them pull at the start of the last substep; every row of
    every substep is finite, with every sentinel (area 18) wet at the start (wet_throughout: at every substep); every body moved"""
    import test_moorings_cpu as TC
    state, rows, T = want
    _, _, taut = TC.wrench(ms, bodies, lines)
    assert (taut == 1).all(), taut
    assert ((T > 0).any(1)).mean() >= 0.5, T
    assert np.isfinite(state).all() and all(np.isfinite(r).all() for _, r, _ in trace)
    for _, r, _ in (trace if wet_throughout else trace[:1]):
        assert (r[:, 3] > 0.99 * 18.0 * nsentinels).all(), r[:, 3]
    assert (_bits(state[:, 0:3]) != _bits(np.asarray(bodies)[:, 0:3])).any(1).all()
