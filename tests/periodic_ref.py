"""Helpers of the periodic-surface tests (tests/test_periodic_cpu.py, tests/test_periodic_gpu.py): the g++ build of the MW_HD functions over a
tiled mesh (tests/periodic_shim.cpp), synthetic meshes that really repeat, the explicit replication of a mesh as one big mesh for the
float64 brute force of tests/surface_ref.py, and query points over tiles, seam strips and tile corners."""
import ctypes as C
import os

import numpy as np

import shim_build
import surface_ref as S
from conftest import REPO

SHIM = os.path.join(REPO, "tests", "periodic_shim.cpp")
f32 = np.float32


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def build_shim(path):
    L = shim_build.strict_f32(SHIM, path)
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    L.ps_period.restype = f
    L.ps_period.argtypes = [i, f]
    L.ps_rest.restype = f
    L.ps_rest.argtypes = [i, f, i]
    L.ps_query.argtypes = [i, f, f, vp, vp, vp, i, i, vp, C.c_int64, i, vp]
    L.ps_velocity.argtypes = [i, f, f, vp, vp, i, vp, C.c_int64, i, vp]
    L.ps_hull_forces.argtypes = [i, f, f, vp, vp, i, vp, i, vp, i, vp, i, vp, vp, vp]
    L.ps_step_bodies.argtypes = [i, f, f, vp, vp, i, vp, i, vp, i, vp, vp, i, vp, f, i, i, vp]
    L.ps_hull_chunks.argtypes = [i, i]
    L.ps_bodies_step_lds.restype = L.ps_bodies_lds_max.restype = C.c_int64
    L.ps_bodies_step_lds.argtypes = [i, i]
    L.ps_bodies_lds_max.argtypes = []
    return L


def period(R, uw):
    """P = float32(R) * float32(uw), as the library computes it"""
    return float(f32(R) * f32(uw))


def query(shim, R, uw, P, vert, norm, white, wstride, mode, xz, iters=0):
    """[n, 8] of sq_query_point; P = 0: the one footprint.  white [R*R] is spread to `wstride` channels as the library's colours are."""
    xz = np.ascontiguousarray(xz, f32)
    out = np.empty((len(xz), 8), f32)
    wh = np.ascontiguousarray(np.repeat(white[:, None], wstride, 1), f32)
    assert shim.ps_query(R, uw, P, _p(vert), _p(norm), _p(wh), wstride, mode, _p(xz), len(xz), iters, _p(out)) == 0
    return out


def query_raw(shim, R, uw, P, vert, norm, colours, wstride, mode, xz, iters=0):
    """query() on the library's own arrays: colours [R*R, wstride] as they are"""
    xz = np.ascontiguousarray(xz, f32)
    out = np.empty((len(xz), 8), f32)
    assert shim.ps_query(R, uw, P, _p(vert), _p(norm), _p(colours), wstride, mode, _p(xz), len(xz), iters, _p(out)) == 0
    return out


def velocity(shim, R, uw, P, vert, vel, mode, xz, iters=0):
    xz = np.ascontiguousarray(xz, f32)
    out = np.empty((len(xz), 4), f32)
    assert shim.ps_velocity(R, uw, P, _p(vert), _p(vel), mode, _p(xz), len(xz), iters, _p(out)) == 0
    return out


def hull_forces(shim, R, uw, P, vert, vel, hull, tris, bodies, coeffs, iters=0):
    """(slab [n, V, 8], rows [n, 8]) of the hull vertex step and the rows summed in the kernels' order"""
    hull, tris = np.ascontiguousarray(hull, f32), np.ascontiguousarray(tris, np.int32)
    bodies, coeffs = np.ascontiguousarray(bodies, f32), np.ascontiguousarray(coeffs, f32)
    slab = np.empty((len(bodies), len(hull), 8), f32)
    rows = np.empty((len(bodies), 8), f32)
    assert shim.ps_hull_forces(R, uw, P, _p(vert), _p(vel), iters, _p(hull), len(hull), _p(tris), len(tris), _p(bodies), len(bodies),
                               _p(coeffs), _p(slab), _p(rows)) == 0
    return slab, rows


def step_bodies(shim, R, uw, P, vert, vel, hull, tris, bodies, mass, coeffs, dt, substeps, plan, iters=0):
    """(new bodies [n, 16], rows [n, 8]) of the substep chain in the order of plan 0 (per substep) or 1 (one launch)"""
    hull, tris = np.ascontiguousarray(hull, f32), np.ascontiguousarray(tris, np.int32)
    b = np.array(bodies, f32, copy=True)
    mass, coeffs = np.ascontiguousarray(mass, f32), np.ascontiguousarray(coeffs, f32)
    rows = np.empty((len(b), 8), f32)
    assert shim.ps_step_bodies(R, uw, P, _p(vert), _p(vel), iters, _p(hull), len(hull), _p(tris), len(tris), _p(b), _p(mass), len(b),
                               _p(coeffs), float(dt), substeps, plan, _p(rows)) == 0
    return b, rows


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---- meshes ---------------------------------------------------------------------------------------------------------------
def periodic_synth(R, uw, fold, seed=0, nwaves=6):
    """surface_ref.synth_mesh with whole numbers of waves per period L = R * uw, so that the mesh really repeats: vertex (a + R, b) of
    the tiling continues the field.  Returns vert, norm, white (float32) and a smooth per-vertex velocity vel [R*R, 3]."""
    rng = np.random.default_rng(seed)
    rc = S.rest_coords(R, uw).astype(np.float64)
    X, Z = np.meshgrid(rc, rc, indexing="ij")
    L = R * uw
    n = rng.integers(-3, 4, (nwaves, 2))
    n[(n == 0).all(1)] = (1, 2)
    k = 2 * np.pi * n / L
    kmag = np.linalg.norm(k, axis=1)
    amp = rng.uniform(0.3, 1.0, nwaves) / kmag
    phi = rng.uniform(0, 2 * np.pi, nwaves)
    h, hx, hz, Sx, Sz, Jxx, Jxz, Jzz = (np.zeros_like(X) for _ in range(8))
    vel = np.zeros(X.shape + (3,))
    for a, (kx, kz), km, p in zip(amp, k, kmag, phi):
        th = kx * X + kz * Z + p
        h += a * np.cos(th)
        hx += -a * kx * np.sin(th)
        hz += -a * kz * np.sin(th)
        Sx += a * kx / km * np.sin(th)
        Sz += a * kz / km * np.sin(th)
        c = a * np.cos(th)
        Jxx += c * kx * kx / km
        Jxz += c * kx * kz / km
        Jzz += c * kz * kz / km
        w = np.sqrt(9.81 * km)
        vel += np.stack([a * w * kx / km * np.cos(th), a * w * np.sin(th), a * w * kz / km * np.cos(th)], -1)
    tr, det = Jxx + Jzz, Jxx * Jzz - Jxz * Jxz
    lam = fold / (tr / 2 + np.sqrt(np.maximum(tr * tr / 4 - det, 0))).max()
    vert = np.stack([X - lam * Sx, h, Z - lam * Sz], -1).reshape(-1, 3).astype(f32)
    nrm = np.stack([-hx, np.ones_like(h), -hz], -1)
    nrm /= np.linalg.norm(nrm, axis=-1, keepdims=True)
    white = np.clip(lam * (Jxx + Jzz), 0, None)
    return vert, nrm.reshape(-1, 3).astype(f32), white.ravel().astype(f32), vel.reshape(-1, 3).astype(f32)


def tiling(R, uw, reps, vert, *fields):
    """The (2 reps + 1)^2 replication of a mesh with its closing row and column as ONE mesh of Rb = (2 reps + 1) R + 1 grid lines per
    side (grid lines g = -reps R ... (reps + 1) R of the tiled surface): vertex g = k R + a is vertex a displaced by k P.  Returns
    Rb, the rest plane [Rb^2, 2] (float32 rest coordinates rest_coord(a) + float32(k) P, as the header defines them), the vertices
    [Rb^2, 3] in float64 and every further per-vertex field replicated alike."""
    P = f32(R) * f32(uw)
    g = np.arange(-reps * R, (reps + 1) * R + 1)
    k, a = g // R, g % R
    rest = (S.rest_coords(R, uw)[a] + k.astype(f32) * P).astype(f32)
    Rb = len(g)
    ai, aj = np.meshgrid(a, a, indexing="ij")
    ki, kj = np.meshgrid(k, k, indexing="ij")
    idx = (ai * R + aj).ravel()
    big = vert[idx].astype(np.float64)
    big[:, 0] += ki.ravel() * float(P)
    big[:, 2] += kj.ravel() * float(P)
    X, Z = np.meshgrid(rest, rest, indexing="ij")
    return (Rb, np.stack([X.ravel(), Z.ravel()], -1), big) + tuple(f[idx] for f in fields)


def water_on(xz, big_vert, tris, *fields):
    """float64 brute force over every triangle of an explicit mesh: for each world point the triangle that holds it (the first of them),
    the height there and every further per-vertex field interpolated alike; hits = how many triangles held the point."""
    hits = S.world_hits(np.asarray(xz, np.float64), big_vert, tris, 1e-9)
    eta = np.full(len(xz), np.nan)
    outs = [np.full((len(xz),) + f.shape[1:], np.nan) for f in fields]
    nhit = np.zeros(len(xz), int)
    for q, (t, w) in enumerate(hits):
        nhit[q] = len(t)
        if len(t):
            tri = tris[t[0]]
            eta[q] = (w[0] * big_vert[tri, 1]).sum()
            for o, f in zip(outs, fields):
                o[q] = (w[0][:, None] * f[tri].astype(np.float64)).sum(0) if f.ndim > 1 else (w[0] * f[tri].astype(np.float64)).sum()
    return (eta, nhit) + tuple(outs)


# ---- points ---------------------------------------------------------------------------------------------------------------
def base_points(R, uw, n, rng, step=None):
    """Points of the base tile [rest(0), rest(0) + P)^2: uniform ones, points in the two seam strips [rest(R-1), rest(0) + P) and points
    within one cell of the four tile corners (inside the tile).  step: round to multiples of it (2^-8 makes the translations exact)."""
    rc = S.rest_coords(R, uw)
    x0, hi, P = float(rc[0]), float(rc[-1]), period(R, uw)
    parts = [rng.uniform(x0, x0 + P, (n, 2))]
    seam = rng.uniform(hi, x0 + P, n // 4)
    along = rng.uniform(x0, x0 + P, n // 4)
    parts += [np.stack([seam, along], 1), np.stack([along, seam], 1)]
    near = np.where(rng.random((n // 4, 2)) < 0.5, rng.uniform(x0, x0 + uw, (n // 4, 2)), rng.uniform(x0 + P - uw, x0 + P, (n // 4, 2)))
    parts.append(near)
    pts = np.concatenate(parts)
    if step:
        pts = np.round(pts / step) * step
        pts = np.where(pts >= x0 + P, pts - step, pts)
        pts = np.where(pts < x0, pts + step, pts)
    return pts.astype(f32)


def tile_points(R, uw, n, rng, tiles=3):
    """base_points scattered over tiles -tiles ... tiles on both axes"""
    pts = base_points(R, uw, n, rng).astype(np.float64)
    k = rng.integers(-tiles, tiles + 1, pts.shape)
    return (pts + k * period(R, uw)).astype(f32)
