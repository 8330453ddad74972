"""numpy float64 reference of the moorings (include/mistral_water.h, csrc/moorings.h), restated independently of the kernels: the line
force as the header's six steps state it, with x - p taken literally, over all bodies and slots at once, and the moored substep as
body_ref.step under the water row plus the mooring wrench.  Rotations are tests/hull_ref.py's."""
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
