"""Helpers of the draught tests (tests/test_draught_cpu.py, tests/test_draught_gpu.py): the g++ build of the hull family on the water
column (tests/draught_shim.cpp: hull_vertex_draught and the rows in the kernels' summation order, restated by hand in tests/hull_order.h), and the
float64 reference -- the composition of two references that exist: column_ref.query_f64 (which locates every layer, then brackets) at
hull_ref.transform's instance vertices gives each vertex its rest depth, water velocity and residual, and hull_ref.forces / forces_terms
clip and integrate them."""
import ctypes as C
import os

import numpy as np

import column_ref as CR
import hull_ref as H
import shim_build
import surface_ref as S
from conftest import REPO

SHIM = os.path.join(REPO, "tests", "draught_shim.cpp")
f32 = np.float32
RHO, G = 1000.0, 9.81


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def build_shim(path):
    L = shim_build.strict_f32(SHIM, path)
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    L.ds_hull_forces.argtypes = [i, f, f, i, vp, vp, vp, i, vp, i, vp, i, vp, i, vp, vp, vp]
    L.ds_step_bodies.argtypes = [i, f, f, i, vp, vp, vp, i, vp, i, vp, i, vp, vp, i, vp, f, i, vp]
    return L


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def coeffs(density=RHO, gravity=G, linear_drag=0.0, quadratic_drag=0.0, velocity_scale=1.0):
    return np.array([density, gravity, linear_drag, quadratic_drag, velocity_scale], f32)


def _layers(R, depths, pos, vel):
    depths = np.ascontiguousarray(depths, f32)
    pos, vel = np.ascontiguousarray(pos, f32), np.ascontiguousarray(vel, f32)
    assert pos.shape == vel.shape == (len(depths), R * R, 3)
    return depths, pos, vel


def forces(shim, R, uw, P, depths, pos, vel, hull, tris, bodies, cf, iters=0):
    """(slab [n, V, 8], rows [n, 8]) of the vertex step on the column and the rows summed in the kernels' order; P = 0: one footprint"""
    depths, pos, vel = _layers(R, depths, pos, vel)
    hull, tris = np.ascontiguousarray(hull, f32), np.ascontiguousarray(tris, np.int32)
    bodies, cf = np.ascontiguousarray(bodies, f32).reshape(-1, 16), np.ascontiguousarray(cf, f32)
    slab = np.empty((len(bodies), len(hull), 8), f32)
    rows = np.empty((len(bodies), 8), f32)
    assert shim.ds_hull_forces(R, uw, P, len(depths), _p(depths), _p(pos), _p(vel), iters, _p(hull), len(hull), _p(tris), len(tris), _p(bodies),
                               len(bodies), _p(cf), _p(slab), _p(rows)) == 0
    return slab, rows


def step(shim, R, uw, P, depths, pos, vel, hull, tris, bodies, mass, cf, dt, substeps, iters=0):
    """(new bodies [n, 16], rows [n, 8] of the last substep) of the substep chain on the column"""
    depths, pos, vel = _layers(R, depths, pos, vel)
    hull, tris = np.ascontiguousarray(hull, f32), np.ascontiguousarray(tris, np.int32)
    b = np.array(bodies, f32, copy=True).reshape(-1, 16)
    mass, cf = np.ascontiguousarray(mass, f32).reshape(-1, 8), np.ascontiguousarray(cf, f32)
    rows = np.empty((len(b), 8), f32)
    assert shim.ds_step_bodies(R, uw, P, len(depths), _p(depths), _p(pos), _p(vel), iters, _p(hull), len(hull), _p(tris), len(tris), _p(b), _p(mass),
                               len(b), _p(cf), float(dt), int(substeps), _p(rows)) == 0
    return b, rows


# ---- the float64 reference ---------------------------------------------------------------------------------------------------------
def column_f64(R, uw, P, depths, pos, vel, hull, bodies):
    """(x [n, V, 3], col [n, V, 12]) float64: the instance vertices and the column query's rows at them"""
    x = H.transform(bodies, hull)
    col = CR.query_f64(R, uw, P, depths, pos, vel, CR.WORLD, x.reshape(-1, 3)).reshape(x.shape[0], x.shape[1], CR.NOUT)
    return x, col


def forces_f64(R, uw, P, depths, pos, vel, hull, tris, bodies, cf, depth="column"):
    """(rows [n, 7], (S_F, S_tau, area) [n, 3], residual [n]) float64.  depth "column": every vertex carries the column's rest depth and
    (drag on) velocity; "surface": eta - y and the column's velocity -- the depth the hull family uses without draught."""
    bodies = np.asarray(bodies, np.float64).reshape(-1, 16)
    x, col = column_f64(R, uw, P, depths, pos, vel, hull, bodies)
    density, gravity, lin, quad, vscale = (float(v) for v in cf)
    rows, scales, res = [], [], []
    for b in range(len(bodies)):
        d = col[b, :, CR.DEPTH] if depth == "column" else col[b, :, CR.ETA] - x[b, :, 1]
        u = col[b, :, CR.UX:CR.UZ + 1] * vscale if (lin or quad) else np.zeros((x.shape[1], 3))
        row, per = H.forces(x[b], d, u, tris, bodies[b], density, gravity, lin, quad, terms=True)
        sf, st = H.term_scales(per)
        rows.append(row)
        scales.append((sf, st, per[:, 3].sum()))
        res.append(col[b, :, CR.RESIDUAL].max())
    return np.array(rows), np.array(scales), np.array(res)


# ---- layers ------------------------------------------------------------------------------------------------------------------------
def rest_vertices(R, uw):
    """the rest mesh [R*R, 3] float64, vertex (i, j) at i * R + j, y = 0"""
    rc = S.rest_coords(R, uw).astype(np.float64)
    X, Z = np.meshgrid(rc, rc, indexing="ij")
    return np.stack([X.ravel(), np.zeros(R * R), Z.ravel()], -1)


def flat_layers(R, uw, L):
    """(pos, vel) [L, R*R, 3] float32 of flat water: every layer is the rest mesh (a layer's y is its height above its own rest level)"""
    rest = rest_vertices(R, uw).astype(f32)
    return np.stack([rest] * L), np.zeros((L, R * R, 3), f32)


def one_wave_layers(R, uw, depths, m, a, phase, gravity=G):
    """(pos, vel, k) of one deep-water component along x on the periodic R x R mesh, wave number k = 2 pi m / (R uw), float64:
    pos_l = (x0 - A_l sin th, A_l cos th, z0), vel_l = A_l w (cos th, sin th, 0), A_l = a e^{-k d_l}, th = k x0 - phase, w = sqrt(g k):
    particles on circles of radius A_l, the analytic field the layers discretise"""
    rest = rest_vertices(R, uw)
    k = 2 * np.pi * m / (R * uw)
    w = np.sqrt(gravity * k)
    th = k * rest[:, 0] - phase
    pos, vel = [], []
    for d in depths:
        A = a * np.exp(-k * float(d))
        pos.append(np.stack([rest[:, 0] - A * np.sin(th), A * np.cos(th), rest[:, 2]], -1))
        vel.append(np.stack([A * w * np.cos(th), A * w * np.sin(th), np.zeros(len(th))], -1))
    return np.stack(pos), np.stack(vel), k


# ---- hulls -------------------------------------------------------------------------------------------------------------------------
SPAR_DRAUGHT = 8.0


def spar():
    """the 2 x 16 x 2 spar: with its reference point on the rest surface its bottom lies at y = -8 (8 vertices, 12 triangles)"""
    return H.box(2.0, 16.0, 2.0)


def pack(p, q=None, v=None, w=None):
    """bodies [n, 16] float32 = p _ | q | v _ | w _"""
    p = np.asarray(p, f32).reshape(-1, 3)
    b = np.zeros((len(p), 16), f32)
    b[:, 0:3] = p
    b[:, 4:8] = [0, 0, 0, 1] if q is None else np.asarray(q, f32).reshape(-1, 4)
    if v is not None:
        b[:, 8:11] = np.asarray(v, f32).reshape(-1, 3)
    if w is not None:
        b[:, 12:15] = np.asarray(w, f32).reshape(-1, 3)
    return b
