"""Helpers of the raycast tests (mw_ocean_raycast, csrc/raycast.h): the g++ build of tests/raycast_shim.cpp, the grid's triangles in id
order, synthetic meshes, tree_ref -- the hierarchy written in numpy from the comment of raycast.h --, the ray families both tiers cast,
triangle_t_f64 -- a float64 Möller–Trumbore over every triangle (numpy) -- and facing_f64."""
import ctypes as C
import os

import numpy as np

import shim_build
import surface_ref as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(REPO, "tests", "raycast_shim.cpp")


def build_shim(path):
    L = shim_build.strict_f32(SHIM, path)
    vp, i64, ci = C.c_void_p, C.c_int64, C.c_int
    L.rc_shim_default_block.restype = ci
    L.rc_shim_default_block.argtypes = []
    L.rc_shim_nodes.restype = i64
    L.rc_shim_nodes.argtypes = [ci, ci]
    L.rc_shim_build.argtypes = [ci, vp, ci, vp]
    L.rc_shim_trace.argtypes = [ci, vp, vp, vp, ci, ci, vp, vp, i64, vp, vp]
    L.rc_shim_cast.argtypes = [ci, vp, vp, vp, ci, ci, vp, i64, vp, vp]
    L.rc_shim_brute.argtypes = [ci, vp, vp, vp, ci, vp, i64, vp, vp]
    L.rc_shim_query_world.argtypes = [ci, C.c_float, vp, vp, vp, ci, vp, i64, ci, vp, vp]
    return L


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


class Mesh:
    """One surface as the library lays it out: vert / norm [R*R, 3], white [R*R * wstride] (channel 0 is read), rest spacing uw."""

    def __init__(self, R, vert, norm, white, wstride=1, uw=1.0):
        self.R, self.wstride, self.uw = int(R), int(wstride), float(uw)
        self.vert = np.ascontiguousarray(vert, np.float32).reshape(-1, 3)
        self.norm = np.ascontiguousarray(norm, np.float32).reshape(-1, 3)
        self.white = np.ascontiguousarray(white, np.float32).reshape(-1)
        assert len(self.vert) == self.R * self.R and len(self.white) == self.R * self.R * self.wstride


def synthetic(R, kind, seed):
    """flat (y = 0 exactly, horizontally displaced), rough (below the fold limit), choppy (folded: overhangs, several hits per ray) or
    far (rough, translated to x = 1e4: the magnitude of a coordinate dwarfs a leaf's extent)"""
    jit, fold = {"flat": (0.2, 0.6), "rough": (0.2, 0.6), "choppy": (1.2, 1.8), "far": (0.2, 0.6)}[kind]
    if R <= 3:  # too small for synth_mesh's waves: random corners around the rest grid
        rng = np.random.default_rng(seed)
        rest = S.rest_plane(R, 1.0).astype(np.float64)
        vert = np.c_[rest[:, 0], rng.uniform(-0.5, 0.5, R * R), rest[:, 1]] + np.c_[rng.uniform(-jit, jit, (R * R, 1)), np.zeros(R * R),
                                                                                   rng.uniform(-jit, jit, (R * R, 1))]
        norm = rng.normal(size=(R * R, 3)) + [0.0, 3.0, 0.0]
        norm /= np.linalg.norm(norm, axis=1, keepdims=True)
        white = rng.uniform(0, 1, R * R)
    else:
        vert, norm, white = S.synth_mesh(R, 1.0, fold, seed=seed)
        vert = vert.astype(np.float64)
    if kind == "flat":
        vert[:, 1] = 0.0
    if kind == "far":
        vert[:, 0] += 1.0e4
    return Mesh(R, vert, norm, white)


PAD = np.float32(2.0 ** -14)   # MW_RC_PAD


def tree_ref(grid, B):
    """(box [nodes, 8] float32, nb, D): the hierarchy of csrc/raycast.h written from its comment, in float32.  grid [S+1, S+1, 3] holds
    the vertices on the grid lines of the S x S cells.  nb = ceil(S / B) leaf blocks a side at level D, 2^D >= nb; leaf (bx, bz) holds
    the exact min and max of the vertices on lines [bx B, min(bx B + B, S)] x [bz B, min(bz B + B, S)], grown per axis by
    p = PAD ((hi - lo) + max(|lo|, |hi|)), every operation rounded to float32; padding leaves are (+inf, -inf); a parent is the min and
    max of its 2 x 2 children; level L is a 2^L x 2^L grid from node (4^L - 1) / 3, row-major; slots 3 and 7 are 0."""
    g = np.ascontiguousarray(grid, np.float32)
    S_ = g.shape[0] - 1
    assert g.shape == (S_ + 1, S_ + 1, 3) and S_ >= 1 and B >= 1
    nb = -(-S_ // B)
    D = (nb - 1).bit_length()
    first = np.arange(nb) * B
    lines = [np.minimum(first + k, S_) for k in range(B + 1)]     # line k of every block, the last block cut at line S
    lo = np.minimum.reduce([g[l] for l in lines])                 # [nb, S+1, 3]: over the block's lines along x ...
    hi = np.maximum.reduce([g[l] for l in lines])
    lo = np.minimum.reduce([lo[:, l] for l in lines])             # ... then along z: [nb, nb, 3]
    hi = np.maximum.reduce([hi[:, l] for l in lines])
    p = PAD * ((hi - lo) + np.maximum(np.abs(lo), np.abs(hi)))
    assert p.dtype == np.float32
    s = 1 << D
    lvl = np.zeros((s, s, 8), np.float32)
    lvl[:, :, 0:3], lvl[:, :, 4:7] = np.inf, -np.inf
    lvl[:nb, :nb, 0:3], lvl[:nb, :nb, 4:7] = lo - p, hi + p
    levels = [lvl]
    while s > 1:
        s >>= 1
        c = levels[0].reshape(s, 2, s, 2, 8)
        lvl = np.zeros((s, s, 8), np.float32)
        lvl[:, :, 0:3], lvl[:, :, 4:7] = c[..., 0:3].min((1, 3)), c[..., 4:7].max((1, 3))
        levels.insert(0, lvl)
    box = np.concatenate([l.reshape(-1, 8) for l in levels])
    assert box.dtype == np.float32 and len(box) == (4 ** (D + 1) - 1) // 3
    return box, nb, D


def shim_tree(L, m, B):
    """the serial build of the shim (rc_build_serial): box [nodes, 8]"""
    box = np.full((L.rc_shim_nodes(m.R, B), 8), np.nan, np.float32)
    assert L.rc_shim_build(m.R, _p(m.vert), B, _p(box)) == 0
    return box


def same_tree(a, b):
    """every node equal as float32 values (no NaN; only the sign of a zero may differ in bits); else the first nodes that differ"""
    if a.shape == b.shape and np.array_equal(a, b):
        return True, None
    if a.shape != b.shape:
        return False, (a.shape, b.shape)
    bad = np.flatnonzero(~(a == b).all(1))
    return False, (len(bad), bad[:6], a[bad[:3]], b[bad[:3]])


def cast(L, m, rays, B=None, brute=False):
    """(out [n, 8], hit [n, 2]) of the shim: the hierarchy with leaf blocks of B cells (None: the library's default), or every
    triangle (brute)"""
    B = L.rc_shim_default_block() if B is None else B
    rays = np.ascontiguousarray(rays, np.float32).reshape(-1, 8)
    n = len(rays)
    out = np.empty((n, 8), np.float32)
    hit = np.empty((n, 2), np.int32)
    if brute:
        rc = L.rc_shim_brute(m.R, _p(m.vert), _p(m.norm), _p(m.white), m.wstride, _p(rays), n, _p(out), _p(hit))
    else:
        rc = L.rc_shim_cast(m.R, _p(m.vert), _p(m.norm), _p(m.white), m.wstride, B, _p(rays), n, _p(out), _p(hit))
    assert rc == 0
    return out, hit


def query_world(L, m, xz, iters=16):
    """world-mode surface query rows [n, 8] (surface_query.h) and the id of the triangle it located (-1: none)"""
    xz = np.ascontiguousarray(xz, np.float32).reshape(-1, 2)
    out = np.empty((len(xz), 8), np.float32)
    tri = np.empty(len(xz), np.int32)
    assert L.rc_shim_query_world(m.R, m.uw, _p(m.vert), _p(m.norm), _p(m.white), m.wstride, _p(xz), len(xz), iters, _p(out), _p(tri)) == 0
    return out, tri


def pack(origins, directions, tmin=0.0, tmax=np.inf):
    o, d = np.asarray(origins, np.float32).reshape(-1, 3), np.asarray(directions, np.float32).reshape(-1, 3)
    t0, t1 = np.asarray(tmin, np.float32).reshape(-1), np.asarray(tmax, np.float32).reshape(-1)
    n = max(len(o), len(d), len(t0), len(t1))
    r = np.empty((n, 8), np.float32)
    r[:, 0:3], r[:, 3], r[:, 4:7], r[:, 7] = o, t0, d, t1
    return r


def id_triangles(R):
    """[2 (R-1)^2, 3] vertex indices, row = triangle id, corners in sq_triangle order"""
    i, j = np.meshgrid(np.arange(R - 1), np.arange(R - 1), indexing="ij")
    c = (i * R + j).ravel()
    lower = np.stack([c, c + R, c + 1], -1)
    upper = np.stack([c + R + 1, c + R, c + 1], -1)
    return np.stack([lower, upper], 1).reshape(-1, 3)


def families(vert, R, rng, n=100):
    """name -> rays [k, 8]: random rays, vertical down / up rays, horizontal rays at vertex heights, rays aimed at vertices and at points
    of shared edges (midpoints included), rays running along shared edges, segments, segments with tmin / tmax windows"""
    v = np.asarray(vert, np.float32).reshape(-1, 3)
    lo, hi = v.min(0).astype(np.float64), v.max(0).astype(np.float64)
    span = max(hi[0] - lo[0], hi[2] - lo[2], 1.0)
    m, h = 0.1 * span, 2.0 + (hi[1] - lo[1])
    box_lo, box_hi = [lo[0] - m, lo[1] - h, lo[2] - m], [hi[0] + m, hi[1] + h, hi[2] + m]

    def origins(k):
        return rng.uniform(box_lo, box_hi, (k, 3)).astype(np.float32)

    f = {}
    f["random"] = pack(origins(n), rng.normal(size=(n, 3)) * rng.uniform(0.1, 10.0, (n, 1)))
    xz = rng.uniform([lo[0], lo[2]], [hi[0], hi[2]], (n, 2))
    f["vertical"] = np.concatenate([pack(np.c_[xz[:, 0], np.full(n, hi[1] + 5), xz[:, 1]], [0.0, -1.0, 0.0]),
                                    pack(np.c_[xz[:, 0], np.full(n, lo[1] - 5), xz[:, 1]], [0.0, 2.5, 0.0])])
    idx = rng.integers(0, R * R, n)
    ang = rng.uniform(0, 2 * np.pi, n)
    c, s = np.cos(ang), np.sin(ang)
    f["grazing"] = pack(np.c_[v[idx, 0] - 2 * span * c, v[idx, 1], v[idx, 2] - 2 * span * s], np.c_[c, np.zeros(n), s])
    o = origins(n)
    f["vertices"] = pack(o, v[rng.integers(0, R * R, n)] - o)
    i, j, kind = rng.integers(0, R - 1, n), rng.integers(0, R - 1, n), rng.integers(0, 3, n)
    a = i * R + j
    b = np.where(kind == 0, a + R, a + 1)                       # along i, along j, or the cell's diagonal (i+1,j)-(i,j+1)
    a = np.where(kind == 2, a + R, a)
    frac = np.where(rng.random(n) < 0.5, 0.5, rng.random(n)).astype(np.float32)[:, None]
    tgt = (v[a] + frac * (v[b] - v[a])).astype(np.float32)
    o = origins(n)
    f["edges"] = pack(o, tgt - o)
    f["along_edges"] = pack(v[a] - 2 * (v[b] - v[a]), v[b] - v[a])
    p0, p1 = origins(n), origins(n)
    f["segments"] = pack(p0, p1 - p0, 0.0, 1.0)
    t0 = rng.uniform(0.0, 0.6, n)
    f["windows"] = pack(p0, p1 - p0, t0, t0 + rng.uniform(0.0, 0.6, n))
    return f


def triangle_t_f64(vert, tris, ray, slack=1e-9):
    """t of the ray on every triangle (float64 Möller–Trumbore, two-sided, barycentric slack), +inf where it misses or t is outside
    [tmin, tmax]"""
    P = np.asarray(vert, np.float64).reshape(-1, 3)[tris]
    a, e1, e2 = P[:, 0], P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]
    o, d = ray[0:3].astype(np.float64), ray[4:7].astype(np.float64)
    pv = np.cross(d, e2)
    det = (e1 * pv).sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / det
        s = o - a
        u = (s * pv).sum(1) * inv
        q = np.cross(s, e1)
        w = (q * d).sum(1) * inv
        t = (e2 * q).sum(1) * inv
        ok = (det != 0) & (u >= -slack) & (w >= -slack) & (u + w <= 1 + slack) & (t >= ray[3]) & (t <= ray[7])
    return np.where(ok, t, np.inf)


def facing_f64(vert, R, tri, d):
    """+1 / -1 of the header's definition for triangle ids tri and directions d [n, 3]: the sign of d . n_g in float64, n_g written
    out from P(i,j) as the header gives it"""
    V = np.asarray(vert, np.float32).reshape(-1, 3).astype(np.float64)
    cell, up = tri >> 1, (tri & 1).astype(bool)
    i, j = cell // (R - 1), cell % (R - 1)
    P = lambda a, b: V[a * R + b]  # noqa: E731
    a_ = np.where(up[:, None], P(i + 1, j + 1), P(i, j))
    e1 = np.where(up[:, None], P(i + 1, j), P(i, j + 1)) - a_
    e2 = np.where(up[:, None], P(i, j + 1), P(i + 1, j)) - a_
    gx = e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1]
    gy = e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2]
    gz = e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]
    d = np.asarray(d, np.float32).astype(np.float64)
    dn = (d[:, 0] * gx + d[:, 1] * gy) + d[:, 2] * gz
    return np.where(dn < 0, 1, -1), dn
