"""numpy float64 reference of mw_ocean_step_bodies' integrator and of mw_hull_mass_properties (include/mistral_water.h,
csrc/rigid_bodies.h), restated independently of the kernels: the substep acts on the world-frame inertia I_w = R I_b R^T as the header
states it (the kernel evaluates the same quantity in body axes), and the mass properties come from signed tetrahedra about the origin.
Hulls and rotations are tests/hull_ref.py's."""
import numpy as np

import hull_ref as H


def inertia_matrix(mass_row):
    """I_b [3, 3] of a mass row (m, Ixx, Iyy, Izz, Ixy, Ixz, Iyz, 0)"""
    _, xx, yy, zz, xy, xz, yz = (float(v) for v in np.asarray(mass_row, np.float64)[:7])
    return np.array([[xx, xy, xz], [xy, yy, yz], [xz, yz, zz]])


def quat_mul(a, b):
    """a (x) b for quaternions (x, y, z, w)"""
    av, aw, bv, bw = a[:3], a[3], b[:3], b[3]
    return np.concatenate([aw * bv + bw * av + np.cross(av, bv), [aw * bw - av @ bv]])


def step(body, row, mass_row, g, h):
    """one substep (header steps 2-5) of body [16] under the row [8] of its state -> the new body [16] (f64); a row with a NaN leaves
    the body as it is"""
    b = np.asarray(body, np.float64).copy()
    row = np.asarray(row, np.float64)
    if np.isnan(row).any():
        return b
    m = float(mass_row[0])
    R = H.rotation(b[4:8])[0]
    Iw = R @ inertia_matrix(mass_row) @ R.T
    b[8:11] = b[8:11] + h * (row[0:3] / m + np.array([0.0, -g, 0.0]))
    w = b[12:15]
    b[12:15] = w + h * np.linalg.solve(Iw, row[4:7] - np.cross(w, Iw @ w))
    b[0:3] = b[0:3] + h * b[8:11]
    q = b[4:8] + 0.5 * h * quat_mul(np.concatenate([b[12:15], [0.0]]), b[4:8])
    b[4:8] = q / np.linalg.norm(q)
    return b


def mass_properties(x, tris, density):
    """(mass, centroid [3], inertia [3, 3] about the centroid, hull axes) of the closed mesh x [V, 3] (outward winding)"""
    x = np.asarray(x, np.float64)
    t = np.asarray(tris)
    a, b, c = x[t[:, 0]], x[t[:, 1]], x[t[:, 2]]
    v = np.einsum("ij,ij->i", a, np.cross(b, c)) / 6
    s = a + b + c
    V = v.sum()
    cen = (v[:, None] * s).sum(0) / 4 / V
    outer = lambda p: np.einsum("ni,nj->nij", p, p)  # noqa: E731
    M2 = np.einsum("n,nij->ij", v / 20, outer(a) + outer(b) + outer(c) + outer(s))  # int x_i x_j dV about the origin
    C = density * (M2 - V * np.outer(cen, cen))
    return density * V, cen, np.trace(C) * np.eye(3) - C


def box_inertia(m, w, h, l):
    """the solid box's tensor about its centre, extent w (x) h (y) l (z)"""
    return np.diag([m * (h * h + l * l) / 12, m * (w * w + l * l) / 12, m * (w * w + h * h) / 12])
