"""Helpers of the water-column tests (tests/test_column_cpu.py, tests/test_column_gpu.py): the g++ build of the MW_HD functions of
csrc/water_column.h (tests/column_shim.cpp), and two float64 references --

(a) layers_f64: the layers of a frame from the oracle.  A layer is the frame pipeline on the attenuated spectrum (A h0, A h0c),
    A = e^{-k d}, and the velocity pipeline on its weighted twin; the attenuation and the weighting are done in float64, the spectrum is
    cast to float32 as tests/velocity_ref.py casts it, and the oracle's float64 transforms do the rest.
(b) query_f64: a numpy restatement of both query modes over given layer arrays.  It locates the point in EVERY layer (an unclamped
    float64 Newton walk over the piecewise-affine map with the exact affine solve per visited triangle) and only then brackets, so the
    device's early exit is checked against it, not assumed."""
import ctypes as C
import os

import numpy as np

import shim_build
import surface_ref as S
import velocity_ref as V
from conftest import REPO
from oracle import oracle as O

SHIM = os.path.join(REPO, "tests", "column_shim.cpp")
f32 = np.float32
REST, WORLD = 0, 1
NOUT = 12
UX, UY, UZ, DEPTH, PX, PY, PZ, LAMBDA, X0, Z0, ETA, RESIDUAL = range(12)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def build_shim(path):
    L = shim_build.strict_f32(SHIM, path)
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    L.cs_query.argtypes = [i, f, f, i, vp, vp, vp, i, vp, C.c_int64, i, vp]
    L.cs_weight.restype = None
    L.cs_weight.argtypes = [i, f, f, f, vp, vp, vp, vp, vp, vp, vp]
    return L


def pad4(xyz):
    """[n, 3] -> the [n, 4] float32 rows the entry points take"""
    a = np.asarray(xyz, f32).reshape(-1, 3)
    q = np.zeros((len(a), 4), f32)
    q[:, :3] = a
    return q


def query(shim, R, uw, P, depths, pos, vel, mode, xyz, iters=0):
    """[n, 12] of col_query_point over layer arrays pos, vel [L, R*R, 3] (float32); P = 0: the one footprint."""
    depths = np.ascontiguousarray(depths, f32)
    pos, vel = np.ascontiguousarray(pos, f32), np.ascontiguousarray(vel, f32)
    assert pos.shape == vel.shape == (len(depths), R * R, 3)
    q = pad4(xyz)
    out = np.empty((len(q), NOUT), f32)
    assert shim.cs_query(R, uw, P, len(depths), _p(depths), _p(pos), _p(vel), mode, _p(q), len(q), iters, _p(out)) == 0
    return out


def weights(shim, p, depth, h0, h0c):
    """(A [N, N], ph0, ph0c, vh0, vh0c [N, N, 2]) of the layer builder at one depth, strict float32"""
    N = p.N
    h0, h0c = np.ascontiguousarray(h0, f32), np.ascontiguousarray(h0c, f32)
    A = np.empty((N, N), f32)
    o = [np.empty((N, N, 2), f32) for _ in range(4)]
    shim.cs_weight(N, p.length, p.gravity, depth, _p(h0), _p(h0c), _p(A), *[_p(a) for a in o])
    return (A, *o)


# ---- (a) layers from the oracle ---------------------------------------------------------------------------------------------------
def wave_number(p):
    """k(n, m) [N, N]: the float32 sequence of omega_f32 (csrc/mw_math.h:147-152) up to the inner square root, as float64"""
    N = p.N
    n = (2 * np.arange(N) - N).astype(f32)
    k1 = (f32(3.1415926536) * n).astype(f32) / f32(p.length)
    k1 = k1.astype(f32)
    s = ((k1 * k1).astype(f32)[:, None] + (k1 * k1).astype(f32)[None, :]).astype(f32)
    return np.sqrt(s).astype(f32).astype(np.float64)


def _evaluator(p):
    return O.eval_fft_f64 if (p.commensurate and p.N % 2 == 0 and p.N >= 8 and (p.N & (p.N - 1)) == 0) else O.eval_matmul_f64


def layers_f64(p, h0, h0c, t, depths):
    """(pos, vel) [L, N*N, 3] float64 of the frame at t: pos_l the oracle's vertices on (A_l h0, A_l h0c) (y = h_l, not h_l - d_l),
    vel_l its velocity on the weighted pair (velocity_ref.weight applied to the attenuated pair), minus the rest mesh."""
    k, w = wave_number(p), V.fftmesh_omega(p)
    ev = _evaluator(p)
    rest = O.rest_mesh(p)[0].astype(np.float64)
    pos, vel = [], []
    for d in depths:
        A = np.exp(-k * float(d))[..., None]
        a, b = A * np.asarray(h0, np.float64), A * np.asarray(h0c, np.float64)
        pos.append(ev(p, a.astype(f32), b.astype(f32), t)[0])
        va, vb = V.weight(a, b, w)
        vel.append(ev(p, va.astype(f32), vb.astype(f32), t)[0] - rest)
    return np.stack(pos), np.stack(vel)


# ---- (b) the queries in float64 ---------------------------------------------------------------------------------------------------
class _Grid:
    """cells, triangles and corners of the R x R mesh in float64; P != 0: the infinite tiling"""

    def __init__(self, R, uw, P):
        self.R, self.uw, self.P = R, float(f32(uw)), float(P)
        self.rc = S.rest_coords(R, uw).astype(np.float64)

    def rest(self, g):
        if self.P == 0.0:
            return self.rc[g]
        return self.rc[np.mod(g, self.R)] + np.floor_divide(g, self.R) * self.P

    def cell(self, x):
        g = np.floor((x - self.rc[0]) / self.uw).astype(np.int64)
        if self.P == 0.0:
            g = np.clip(g, 0, self.R - 2)
        for _ in range(2):
            lo, hi = self.rest(g), self.rest(g + 1)
            step = np.where(x < lo, -1, np.where(x > hi, 1, 0))
            if self.P == 0.0:
                step = np.where((g + step < 0) | (g + step > self.R - 2), 0, step)
            g = g + step
        lo, hi = self.rest(g), self.rest(g + 1)
        return g, (x - lo) / (hi - lo)

    def triangle(self, gi, gj, fa, fb):
        """corners (grid lines [n, 3] per axis) and weights [n, 3] of the triangle of cell (gi, gj) holding (fa, fb)"""
        up = fa + fb > 1.0
        ci = np.where(up[:, None], np.stack([gi + 1, gi + 1, gi], -1), np.stack([gi, gi + 1, gi], -1))
        cj = np.where(up[:, None], np.stack([gj + 1, gj, gj + 1], -1), np.stack([gj, gj, gj + 1], -1))
        w = np.where(up[:, None], np.stack([fa + fb - 1.0, 1.0 - fb, 1.0 - fa], -1), np.stack([1.0 - fa - fb, fa, fb], -1))
        return up, ci, cj, w

    def corners(self, arr, ci, cj):
        """arr [R*R, 3] at the corners [n, 3, 3], without the tile shift"""
        R = self.R
        return arr[np.mod(ci, R) * R + np.mod(cj, R)] if self.P else arr[ci * R + cj]

    def shift(self, ci, cj):
        if self.P == 0.0:
            return np.zeros(ci.shape), np.zeros(cj.shape)
        return np.floor_divide(ci, self.R) * self.P, np.floor_divide(cj, self.R) * self.P


def _locate_world(G, pos, qx, qz, iters=200):
    """float64 walk on the displaced map of pos: returns (ci, cj, w, residual) per point"""
    n = len(qx)
    lo, hi = G.rc[0], G.rc[-1]
    ux, uz = qx.copy(), qz.copy()
    if G.P == 0.0:
        ux, uz = np.clip(ux, lo, hi), np.clip(uz, lo, hi)
    best = np.full(n, np.inf)
    out_ci, out_cj, out_w = np.zeros((n, 3), np.int64), np.zeros((n, 3), np.int64), np.zeros((n, 3))
    act = np.arange(n)
    for it in range(iters + 1):
        if len(act) == 0:
            break
        x, z = ux[act], uz[act]
        gi, ta = G.cell(x)
        gj, tb = G.cell(z)
        up, ci, cj, w = G.triangle(gi, gj, ta, tb)
        sx, sz = G.shift(ci, cj)
        c = G.corners(pos, ci, cj)
        px, pz = c[:, :, 0] + sx, c[:, :, 2] + sz
        # P(fa, fb) = O + fa ea + fb eb in the cell's local coordinates
        ox = np.where(up, px[:, 1] + px[:, 2] - px[:, 0], px[:, 0]); oz = np.where(up, pz[:, 1] + pz[:, 2] - pz[:, 0], pz[:, 0])
        ax = np.where(up, px[:, 0] - px[:, 2], px[:, 1] - px[:, 0]); az = np.where(up, pz[:, 0] - pz[:, 2], pz[:, 1] - pz[:, 0])
        bx = np.where(up, px[:, 0] - px[:, 1], px[:, 2] - px[:, 0]); bz = np.where(up, pz[:, 0] - pz[:, 1], pz[:, 2] - pz[:, 0])
        rx, rz = qx[act] - ox, qz[act] - oz
        det = ax * bz - bx * az
        with np.errstate(divide="ignore", invalid="ignore"):
            sa, sb = (rx * bz - bx * rz) / det, (ax * rz - rx * az) / det
        tol = 1e-12
        inside = np.where(up, (sa <= 1 + tol) & (sb <= 1 + tol) & (sa + sb >= 1 - tol), (sa >= -tol) & (sb >= -tol) & (sa + sb <= 1 + tol))
        ex, ez = (w * px).sum(-1) - qx[act], (w * pz).sum(-1) - qz[act]
        r = np.hypot(ex, ez)
        better = ~inside & (r < best[act])
        k = act[better]
        best[k] = r[better]; out_ci[k] = ci[better]; out_cj[k] = cj[better]; out_w[k] = w[better]
        if inside.any():
            fa, fb = np.clip(sa[inside], 0, 1), np.clip(sb[inside], 0, 1)
            upi = up[inside]
            wi = np.where(upi[:, None], np.stack([fa + fb - 1.0, 1.0 - fb, 1.0 - fa], -1), np.stack([1.0 - fa - fb, fa, fb], -1))
            k = act[inside]
            out_ci[k] = ci[inside]; out_cj[k] = cj[inside]; out_w[k] = wi
            best[k] = np.hypot((wi * px[inside]).sum(-1) - qx[k], (wi * pz[inside]).sum(-1) - qz[k])
        go = ~inside
        da, db = sa - ta, sb - tb
        ln = np.maximum(np.abs(da), np.abs(db))
        newton = go & (det > 0) & (ln <= 1e30)
        sc = np.where(ln > 4.0, 4.0 / np.where(ln > 0, ln, 1.0), 1.0)
        nx = np.where(newton, x + np.nan_to_num(da * sc) * G.uw, x - ex)
        nz = np.where(newton, z + np.nan_to_num(db * sc) * G.uw, z - ez)
        if G.P == 0.0:
            nx, nz = np.clip(nx, lo, hi), np.clip(nz, lo, hi)
        ux[act], uz[act] = nx, nz
        act = act[go]
    return out_ci, out_cj, out_w, best


def _gather(G, pos, vel, d, ci, cj, w):
    """(u [n, 3], p [n, 3] with y = h - d, x0, z0) of one layer at located corners, in the frame of the locate"""
    sx, sz = G.shift(ci, cj)
    c = G.corners(pos, ci, cj).astype(np.float64).copy()
    c[:, :, 0] += sx
    c[:, :, 2] += sz
    p = (w[:, :, None] * c).sum(1)
    p[:, 1] -= d
    u = (w[:, :, None] * G.corners(vel, ci, cj)).sum(1)
    return u, p, (w * G.rest(ci)).sum(-1), (w * G.rest(cj)).sum(-1)


def layer_heights_f64(R, uw, P, depths, pos, xz):
    """Y [L, n]: the height h_l - d_l of every layer over the world points xz [n, 2] (inside the base tile when P != 0), float64"""
    G = _Grid(R, uw, P)
    xz = np.asarray(xz, np.float64)
    Y = []
    for l, d in enumerate(depths):
        ci, cj, w, _ = _locate_world(G, np.asarray(pos[l], np.float64), xz[:, 0].copy(), xz[:, 1].copy())
        Y.append((w * G.corners(np.asarray(pos[l], np.float64), ci, cj)[:, :, 1]).sum(-1) - float(d))
    return np.stack(Y)


def query_f64(R, uw, P, depths, pos, vel, mode, xyz):
    """[n, 12] float64 of the column query over pos, vel [L, R*R, 3]; every layer is located, then the point is bracketed.  Rows the rules
    make NaN are NaN."""
    depths = np.asarray(depths, np.float64)
    pos, vel = np.asarray(pos, np.float64), np.asarray(vel, np.float64)
    q = np.asarray(xyz, np.float64).reshape(-1, 3)
    n, L = len(q), len(depths)
    out = np.full((n, NOUT), np.nan)
    G = _Grid(R, uw, P)
    good = np.isfinite(q).all(-1)
    kx = kz = np.zeros(n)
    x, z = q[:, 0].copy(), q[:, 2].copy()
    if P:
        with np.errstate(invalid="ignore"):
            kx, kz = np.floor((x - G.rc[0]) / P), np.floor((z - G.rc[0]) / P)
        kx, kz = np.where(good, kx, 0.0), np.where(good, kz, 0.0)
        x, z = x - kx * P, z - kz * P
    x, z = np.where(good, x, 0.0), np.where(good, z, 0.0)
    mix = lambda s, a, b: (1.0 - s) * a + s * b
    if mode == REST:
        d = q[:, 1]
        with np.errstate(invalid="ignore"):
            good &= (d >= 0) & (d <= depths[-1])
            if not P:
                good &= (x >= G.rc[0]) & (x <= G.rc[-1]) & (z >= G.rc[0]) & (z <= G.rc[-1])
        gi, fa = G.cell(np.where(good, x, 0.0))
        gj, fb = G.cell(np.where(good, z, 0.0))
        _, ci, cj, w = G.triangle(gi, gj, fa, fb)
        lay = [_gather(G, pos[l], vel[l], depths[l], ci, cj, w) for l in range(L)]
        l = np.clip(np.searchsorted(depths, np.where(good, d, 0.0), side="right") - 1, 0, L - 2)
        s = (np.where(good, d, 0.0) - depths[l]) / (depths[l + 1] - depths[l])
        pick = lambda k, dl: np.stack([lay[m][k] for m in range(L)])[l + dl, np.arange(n)]
        out[:, UX:UZ + 1] = mix(s[:, None], pick(0, 0), pick(0, 1))
        out[:, PX:PZ + 1] = mix(s[:, None], pick(1, 0), pick(1, 1))
        out[:, X0] = mix(s, pick(2, 0), pick(2, 1))
        out[:, Z0] = mix(s, pick(3, 0), pick(3, 1))
        out[:, DEPTH], out[:, LAMBDA], out[:, ETA], out[:, RESIDUAL] = d, l + s, lay[0][1][:, 1], 0.0
    else:
        y = q[:, 1]
        lay, res = [], []
        for l in range(L):
            ci, cj, w, r = _locate_world(G, pos[l], x, z)
            lay.append(_gather(G, pos[l], vel[l], depths[l], ci, cj, w))
            res.append(r)
        Y = np.stack([lay[l][1][:, 1] for l in range(L)])
        res = np.stack(res)
        todo = good.copy()
        air = todo & (y > Y[0])
        out[air, UX:UZ + 1] = 0.0
        out[air, PX:PZ + 1] = lay[0][1][air]
        out[air, X0], out[air, Z0] = lay[0][2][air], lay[0][3][air]
        out[air, DEPTH], out[air, LAMBDA], out[air, RESIDUAL] = (Y[0] - y)[air], 0.0, res[0][air]
        todo &= ~air
        for l in range(L):
            on = todo & (y == Y[l])   # exactly on layer l (never, for all practical purposes, with float64 heights): its sample
            for c0, k in ((UX, 0), (PX, 1)):
                out[on, c0:c0 + 3] = lay[l][k][on]
            out[on, X0], out[on, Z0], out[on, DEPTH], out[on, LAMBDA] = lay[l][2][on], lay[l][3][on], depths[l], l
            out[on, RESIDUAL] = res[:l + 1, on].max(0)
            todo &= ~on
            if l == L - 1:
                break
            hit = todo & (y > Y[l + 1])
            s = ((Y[l] - y) / np.where(hit, Y[l] - Y[l + 1], 1.0))[hit]
            for c0, k in ((UX, 0), (PX, 1)):
                out[hit, c0:c0 + 3] = mix(s[:, None], lay[l][k][hit], lay[l + 1][k][hit])
            out[hit, X0] = mix(s, lay[l][2][hit], lay[l + 1][2][hit])
            out[hit, Z0] = mix(s, lay[l][3][hit], lay[l + 1][3][hit])
            out[hit, DEPTH], out[hit, LAMBDA] = mix(s, depths[l], depths[l + 1]), l + s
            out[hit, RESIDUAL] = res[:l + 2, hit].max(0)
            todo &= ~hit
        for c0, k in ((UX, 0), (PX, 1)):
            out[todo, c0:c0 + 3] = lay[L - 1][k][todo]
        out[todo, X0], out[todo, Z0] = lay[L - 1][2][todo], lay[L - 1][3][todo]
        out[todo, DEPTH], out[todo, LAMBDA] = depths[-1] + (Y[-1] - y)[todo], L - 1
        out[todo, RESIDUAL] = res[:, todo].max(0)
        out[:, ETA] = Y[0]
    if P:
        out[:, PX] += kx * P; out[:, X0] += kx * P
        out[:, PZ] += kz * P; out[:, Z0] += kz * P
    out[~good] = np.nan
    return out
