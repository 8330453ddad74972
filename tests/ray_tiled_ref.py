"""Helpers of the tiled raycast tests (mw_ocean_raycast_tiled, csrc/raycast_tiled.h): the g++ build of tests/raycast_tiled_shim.cpp,
synthetic N x N frames (any displacement of the rest grid tiles by construction), a tile's grid lines for ray_ref.tree_ref, the ray families both tiers cast, the comparison
with the brute force and the float64 view of a window's triangle instances."""
import ctypes as C
import os

import numpy as np

import shim_build
from ray_ref import _p, pack

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(REPO, "tests", "raycast_tiled_shim.cpp")
OUT_OF_REACH = -2


def build_shim(path):
    L = shim_build.strict_f32(SHIM, path)
    vp, i64, ci, cf = C.c_void_p, C.c_int64, C.c_int, C.c_float
    L.rct_shim_max_reach.restype = ci
    L.rct_shim_nodes.restype = i64
    L.rct_shim_nodes.argtypes = [ci, ci]
    L.rct_shim_build.argtypes = [ci, cf, cf, vp, ci, vp]
    L.rct_shim_root.argtypes = [ci, cf, cf, vp, ci, vp, vp, vp]
    L.rct_shim_overhang.argtypes = [ci, cf, cf, vp]
    L.rct_shim_cast.argtypes = [ci, cf, cf, vp, vp, vp, ci, ci, ci, vp, i64, vp, vp]
    L.rct_shim_brute.argtypes = [ci, cf, cf, vp, vp, vp, ci, ci, vp, i64, vp, vp]
    return L


def rest(N, uw):
    """rest_coord(N, uw, a) for a = 0 .. N-1 (csrc/mw_math.h), float32"""
    a = np.arange(N, dtype=np.int64) - N // 2
    base = a.astype(np.float32) * np.float32(uw)
    return base + np.float32(uw) / np.float32(2) if N % 2 == 0 else base


class TMesh:
    """One frame read as its tiling: vert / norm [N*N, 3], white [N*N * wstride], rest spacing uw, period P = float32(N) * uw."""

    def __init__(self, N, vert, norm, white, wstride=1, uw=1.0):
        self.N, self.wstride, self.uw = int(N), int(wstride), float(np.float32(uw))
        self.P = float(np.float32(N) * np.float32(uw))
        self.vert = np.ascontiguousarray(vert, np.float32).reshape(-1, 3)
        self.norm = np.ascontiguousarray(norm, np.float32).reshape(-1, 3)
        self.white = np.ascontiguousarray(white, np.float32).reshape(-1)
        self.x0 = float(rest(self.N, self.uw)[0])
        assert len(self.vert) == self.N * self.N and len(self.white) == self.N * self.N * self.wstride


def synthetic(N, kind, seed, uw=1.0):
    """flat: the rest grid at y = 0.25; rough: heights and a horizontal displacement below half a cell; folded: horizontal displacement
    of up to 1.5 cells (triangles fold over); big: some vertices displaced horizontally by more than a period (h = 2); level: rough
    with y = 0 exactly; far: rough, translated to x = 1e4 (the magnitude of a coordinate dwarfs a leaf's extent)"""
    rng = np.random.default_rng(seed)
    r = rest(N, uw).astype(np.float64)
    X, Z = np.meshgrid(r, r, indexing="ij")
    amp = {"flat": 0.0, "rough": 0.45, "folded": 1.5, "big": 0.45, "level": 0.45, "far": 0.45}[kind] * uw
    dx, dz = rng.uniform(-amp, amp, (2, N, N))
    y = np.full((N, N), 0.25) if kind == "flat" else rng.uniform(-1.0, 1.0, (N, N)) * max(uw, 0.5)
    if kind == "level":
        y = np.zeros((N, N))
    if kind == "far":
        dx += 1.0e4
    if kind == "big":
        P = N * uw
        k = rng.integers(0, N * N, max(1, N * N // 8))
        dx.ravel()[k] += rng.choice([-1.2, 1.2], len(k)) * P
        dz.ravel()[k[: len(k) // 2]] += rng.choice([-1.1, 1.1], len(k) // 2) * P
    vert = np.stack([X + dx, y, Z + dz], -1).reshape(-1, 3)
    norm = rng.normal(size=(N * N, 3)) * 0.3 + [0.0, 1.0, 0.0]
    return TMesh(N, vert, norm, rng.random(N * N), uw=uw)


def root(L, m, B=2):
    """(lo [3], hi [3], h) of the shim's root box: h = the tiles a tile's geometry can overhang"""
    r6, x0, h = np.empty(6, np.float32), C.c_float(0), C.c_int32(0)
    assert L.rct_shim_root(m.N, m.uw, m.P, _p(m.vert), B, _p(r6), C.byref(x0), C.byref(h)) == 0
    return r6[:3].copy(), r6[3:].copy(), int(h.value)


def overhang_tiles(L, m, lo, hi):
    """rct_overhang_tiles of a root box (lo [3], hi [3]) of frame m"""
    r6 = np.ascontiguousarray(np.r_[lo, hi], np.float32)
    return int(L.rct_shim_overhang(m.N, m.uw, m.P, _p(r6)))


def tile_grid(m):
    """[N+1, N+1, 3] float32: the vertices on the grid lines of one tile's N x N cells, line N = line 0 with x + 1*P (or z), the
    expression of sq_shift"""
    N, P = m.N, np.float32(m.P)
    g = np.empty((N + 1, N + 1, 3), np.float32)
    g[:N, :N] = m.vert.reshape(N, N, 3)
    g[N, :N] = g[0, :N]
    g[N, :N, 0] = g[0, :N, 0] + np.float32(1) * P
    g[:, N] = g[:, 0]
    g[:, N, 2] = g[:, 0, 2] + np.float32(1) * P
    return g


def shim_tree(L, m, B):
    """the serial build of the shim (rct_build_serial): box [nodes, 8]"""
    box = np.full((L.rct_shim_nodes(m.N, B), 8), np.nan, np.float32)
    assert L.rct_shim_build(m.N, m.uw, m.P, _p(m.vert), B, _p(box)) == 0
    return box


def cast(L, m, rays, reach, B=2, brute=False):
    """(out [n, 8], hit [n, 4]) of the shim: the column walk with leaf blocks of B cells, or every triangle of every window tile"""
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    n = len(rays)
    out = np.empty((n, 8), np.float32)
    hit = np.empty((n, 4), np.int32)
    if brute:
        rc = L.rct_shim_brute(m.N, m.uw, m.P, _p(m.vert), _p(m.norm), _p(m.white), m.wstride, reach, _p(rays), n, _p(out), _p(hit))
    else:
        rc = L.rct_shim_cast(m.N, m.uw, m.P, _p(m.vert), _p(m.norm), _p(m.white), m.wstride, B, reach, _p(rays), n, _p(out), _p(hit))
    assert rc == 0
    return out, hit


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same_rows(out, hit, bo, bh):
    """per ray: the whole row equals the brute force's, bit for bit; an out-of-reach row counts as the brute force's miss"""
    h = hit.copy()
    h[h[:, 0] == OUT_OF_REACH, 0] = -1
    return (bits(out) == bits(bo)).all(1) & (h == bh).all(1)


def shifted(m, v, kx, kz):
    """float32 positions of frame vertices v in relative tile (kx, kz): sq_shift on x and z"""
    p = m.vert[v].copy()
    P = np.float32(m.P)
    kx, kz = np.broadcast_to(kx, p.shape[:-1]), np.broadcast_to(kz, p.shape[:-1])
    p[..., 0] = np.where(kx != 0, p[..., 0] + kx.astype(np.float32) * P, p[..., 0])
    p[..., 2] = np.where(kz != 0, p[..., 2] + kz.astype(np.float32) * P, p[..., 2])
    return p


def tile_triangles(m):
    """(v [2 N^2, 3] frame vertex indices, wi, wj [2 N^2, 3] 0 / 1: the corner lies on the next tile's first grid line), row = tiled id"""
    N = m.N
    i, j = [a.ravel() for a in np.meshgrid(np.arange(N), np.arange(N), indexing="ij")]
    ci = np.stack([np.stack([i, i + 1, i], -1), np.stack([i + 1, i + 1, i], -1)], 1).reshape(-1, 3)
    cj = np.stack([np.stack([j, j, j + 1], -1), np.stack([j + 1, j, j + 1], -1)], 1).reshape(-1, 3)
    wi, wj = (ci == N).astype(np.int64), (cj == N).astype(np.int64)
    return (ci % N) * N + (cj % N), wi, wj


def window_triangles(m, reach):
    """float32 corners [T, 3, 3] of every triangle of the window's tiles around tile 0, and (kx, kz, id) [T, 3] of each"""
    v, wi, wj = tile_triangles(m)
    ks = np.arange(-reach, reach + 1)
    P, K = [], []
    for kx in ks:
        for kz in ks:
            P.append(shifted(m, v, kx + wi, kz + wj))
            K.append(np.stack([np.full(len(v), kx), np.full(len(v), kz), np.arange(len(v))], -1))
    return np.concatenate(P), np.concatenate(K)


def families(m, rng, n=60, far=1000):
    """name -> rays [k, 8]: random rays, vertical rays, horizontal rays at vertex heights, rays at seam vertices and at points of seam
    edges, windows, shallow rays, rays down a tile-boundary plane, and random rays whose origin sits `far` tiles out"""
    N, P, x0 = m.N, m.P, m.x0
    v = m.vert.astype(np.float64)
    ylo, yhi = v[:, 1].min(), v[:, 1].max()
    hgt = 1.0 + (yhi - ylo)

    def origins(k, tiles=1.5):
        c = x0 + P / 2
        return rng.uniform([c - tiles * P, ylo - hgt, c - tiles * P], [c + tiles * P, yhi + hgt, c + tiles * P], (k, 3)).astype(np.float32)

    tt = []   # tile_triangles(m), made once

    def seam_points(k, frac):
        """points of the edges of seam cells (ai or aj = N-1) of the tiles around tile 0: corner e of a triangle towards the next corner"""
        if not tt:
            tt.extend(tile_triangles(m))
        tv, wi, wj = tt
        cell = np.arange(2 * N * N) // 2
        t = rng.choice(np.flatnonzero((cell // N == N - 1) | (cell % N == N - 1)), k)
        kx, kz, e = rng.integers(-1, 2, k), rng.integers(-1, 2, k), rng.integers(0, 3, k)
        e2 = (e + 1) % 3
        A = shifted(m, tv[t, e], kx + wi[t, e], kz + wj[t, e]).astype(np.float64)
        B = shifted(m, tv[t, e2], kx + wi[t, e2], kz + wj[t, e2]).astype(np.float64)
        return (A + frac[:, None] * (B - A)).astype(np.float32)

    f = {}
    f["random"] = pack(origins(n), rng.normal(size=(n, 3)) * rng.uniform(0.1, 10.0, (n, 1)))
    xz = rng.uniform(x0 - P, x0 + 2 * P, (n, 2))
    f["vertical"] = np.concatenate([pack(np.c_[xz[:, 0], np.full(n, yhi + 5), xz[:, 1]], [0.0, -1.0, 0.0]),
                                    pack(np.c_[xz[:, 0], np.full(n, ylo - 5), xz[:, 1]], [0.0, 2.5, 0.0])])
    idx, ang = rng.integers(0, N * N, n), rng.uniform(0, 2 * np.pi, n)
    c, s = np.cos(ang), np.sin(ang)
    f["grazing"] = pack(np.c_[v[idx, 0] - 1.5 * P * c, v[idx, 1], v[idx, 2] - 1.5 * P * s], np.c_[c, np.zeros(n), s])
    o = origins(n)
    f["seam_vertices"] = pack(o, seam_points(n, np.zeros(n)) - o)
    o = origins(n)
    f["seam_edges"] = pack(o, seam_points(n, np.where(rng.random(n) < 0.5, 0.5, rng.random(n))) - o)
    p0, p1, t0 = origins(n), origins(n), rng.uniform(0.0, 0.6, n)
    f["windows"] = pack(p0, p1 - p0, t0, t0 + rng.uniform(0.0, 0.9, n))
    ang = rng.uniform(0, 2 * np.pi, n)
    o = origins(n, 0.5)
    o[:, 1] = yhi + rng.uniform(0.05, 1.0, n)
    f["shallow"] = pack(o, np.c_[np.cos(ang), -rng.uniform(0.01, 0.3, n), np.sin(ang)])
    o = origins(n)
    axis, k = rng.integers(0, 2, n), rng.integers(-1, 3, n)
    plane = (np.float32(x0) + k.astype(np.float32) * np.float32(P)).astype(np.float32)
    d = rng.normal(size=(n, 3))
    o[np.arange(n), 2 * axis] = plane
    d[np.arange(n), 2 * axis] = 0.0
    d[:, 1] = -np.abs(d[:, 1]) * np.where(o[:, 1] > yhi, 1, -1)
    f["boundary_plane"] = pack(o, d)
    o = origins(n).astype(np.float64)
    o[:, [0, 2]] += rng.choice([-far, far], (n, 2)) * P
    f["far"] = pack(o, rng.normal(size=(n, 3)) * [1.0, 0.4, 1.0])
    return f
