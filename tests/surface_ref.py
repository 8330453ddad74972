"""numpy brute-force reference of mw_ocean_query_surface (include/mistral_water.h, csrc/surface_query.h) and synthetic displaced meshes.

The surface is the displaced triangle mesh: vertices [R*R][3] (vertex (i, j) at i*R + j), the triangles of the rest mesh's index buffer,
barycentric interpolation in REST-plane coordinates.  The reference finds, for every query, EVERY triangle that contains it -- in the rest
plane (rest mode) or in the displaced horizontal plane (world mode) -- in float64, so the tests can tell unique answers from folds."""
import numpy as np

f32 = np.float32


def rest_coords(R, uw):
    """rest_coord(R, uw, a) of csrc/mw_math.h in float32: (a - R/2) * uw (+ uw/2 for even R)."""
    base = (np.arange(R) - R // 2).astype(f32) * f32(uw)
    return (base + f32(uw) / f32(2)).astype(f32) if R % 2 == 0 else base


def grid_triangles(R, cells=None):
    """Triangles of rest-grid cells (i, j) split along (i, j+1)-(i+1, j), corner order of the index buffer (S/FFTMesh.cs:120-131):
    lower (i,j) (i,j+1) (i+1,j), upper (i+1,j) (i,j+1) (i+1,j+1).  cells: (ci, cj) arrays (default: all)."""
    if cells is None:
        ci, cj = np.meshgrid(np.arange(R - 1), np.arange(R - 1), indexing="ij")
        ci, cj = ci.ravel(), cj.ravel()
    else:
        ci, cj = cells
    c = ci * R + cj
    lower = np.stack([c, c + 1, c + R], -1)
    upper = np.stack([c + R, c + 1, c + R + 1], -1)
    return np.concatenate([lower, upper]).astype(np.int64)


def _bary(qx, qz, P):
    """P [T,3,2] float64, q [m] -> weights [m,T,3] (NaN for degenerate triangles)."""
    a, b, c = P[:, 0], P[:, 1], P[:, 2]
    v0, v1 = b - a, c - a
    d = v0[:, 0] * v1[:, 1] - v1[:, 0] * v0[:, 1]
    with np.errstate(divide="ignore", invalid="ignore"):
        v2x = qx[:, None] - a[None, :, 0]
        v2z = qz[:, None] - a[None, :, 1]
        wb = (v2x * v1[None, :, 1] - v1[None, :, 0] * v2z) / d[None]
        wc = (v0[None, :, 0] * v2z - v2x * v0[None, :, 1]) / d[None]
    return np.stack([1.0 - wb - wc, wb, wc], -1)


def _interp(tri, w, vert, norm, white):
    """tri [3] vertex ids, w [3] -> (p[3], n[3], white)"""
    p = (w[:, None] * vert[tri].astype(np.float64)).sum(0)
    n = (w[:, None] * norm[tri].astype(np.float64)).sum(0)
    return p, n / np.linalg.norm(n), float((w * white[tri].astype(np.float64)).sum())


def containing(qx, qz, plane_xz, tris, tol):
    """For every query the triangles whose min barycentric weight >= -tol in plane_xz ([R*R,2]) -> list of (tri ids, weights)."""
    P = plane_xz[tris].astype(np.float64)
    out = []
    for s in range(0, len(qx), 128):
        W = _bary(np.asarray(qx[s:s + 128], np.float64), np.asarray(qz[s:s + 128], np.float64), P)
        inside = np.nan_to_num(W.min(-1), nan=-1.0) >= -tol
        for r in range(W.shape[0]):
            t = np.nonzero(inside[r])[0]
            out.append((t, W[r, t]))
    return out


def rest_plane(R, uw):
    rc = rest_coords(R, uw)
    X, Z = np.meshgrid(rc, rc, indexing="ij")
    return np.stack([X.ravel(), Z.ravel()], -1)


def rest_reference(xz, vert, norm, white, R, uw, tris):
    """[n,7] (p, n, white) of rest-mode queries; NaN off the footprint."""
    hits = containing(xz[:, 0], xz[:, 1], rest_plane(R, uw), tris, 1e-9)
    ref = np.full((len(xz), 7), np.nan)
    for k, (t, w) in enumerate(hits):
        if len(t):
            p, n, wh = _interp(tris[t[0]], w[0], vert, norm, white)
            ref[k] = np.concatenate([p, n, [wh]])
    return ref


def world_hits(xz, vert, tris, tol):
    return containing(xz[:, 0], xz[:, 1], vert[:, [0, 2]], tris, tol)


def on_mesh(res, vert, tris, tol_xz, tol_y):
    """True when the point res[0:3] lies on some displaced triangle: its xz inside the triangle (up to tol_xz in barycentric weight)
    and its y the triangle's height there (up to tol_y)."""
    hits = containing(np.array([res[0]]), np.array([res[2]]), vert[:, [0, 2]], tris, tol_xz)[0]
    for t, w in zip(*hits):
        y = float((w * vert[tris[t], 1].astype(np.float64)).sum())
        if abs(y - res[1]) <= tol_y:
            return True
    return False


def synth_mesh(R, uw, fold, seed=0, nwaves=6):
    """A choppy displaced mesh: height h = sum a cos(k.x + phi), horizontal displacement D = -lam sum a khat sin(k.x + phi), with lam
    chosen so that the smallest eigenvalue of I + dD/dx over the vertices is 1 - fold (fold < 1: below the fold limit; > 1: folded).
    Returns vert [R*R,3], norm [R*R,3], white [R*R] (float32)."""
    rng = np.random.default_rng(seed)
    rc = rest_coords(R, uw).astype(np.float64)
    X, Z = np.meshgrid(rc, rc, indexing="ij")
    L = R * uw
    ang = rng.uniform(0, 2 * np.pi, nwaves)
    kmag = 2 * np.pi / (L / rng.uniform(2.0, 7.0, nwaves))
    amp = rng.uniform(0.3, 1.0, nwaves) / kmag
    phi = rng.uniform(0, 2 * np.pi, nwaves)
    h = np.zeros_like(X)
    Sx, Sz, Jxx, Jxz, Jzz, hx, hz = (np.zeros_like(X) for _ in range(7))
    for a, km, t, p in zip(amp, kmag, ang, phi):
        kx, kz = km * np.cos(t), km * np.sin(t)
        th = kx * X + kz * Z + p
        h += a * np.cos(th)
        hx += -a * kx * np.sin(th)
        hz += -a * kz * np.sin(th)
        Sx += a * np.cos(t) * np.sin(th)
        Sz += a * np.sin(t) * np.sin(th)
        c = a * np.cos(th)
        Jxx += c * np.cos(t) * kx
        Jxz += c * np.cos(t) * kz
        Jzz += c * np.sin(t) * kz
    # eigenvalues of the (symmetric) Jacobian of S; D = -lam S, I + dD = I - lam J
    tr, det = Jxx + Jzz, Jxx * Jzz - Jxz * Jxz
    emax = (tr / 2 + np.sqrt(np.maximum(tr * tr / 4 - det, 0))).max()
    lam = fold / emax
    Dx, Dz = -lam * Sx, -lam * Sz
    vert = np.stack([X + Dx, h, Z + Dz], -1).reshape(-1, 3).astype(f32)
    n = np.stack([-hx, np.ones_like(h), -hz], -1)
    n /= np.linalg.norm(n, axis=-1, keepdims=True)
    white = np.clip(lam * (Jxx + Jzz), 0, None)
    return vert, n.reshape(-1, 3).astype(f32), white.ravel().astype(f32)


def all_triangles(R):
    """tris_for of check_world: every triangle of the mesh (brute force)"""
    tris = grid_triangles(R)
    return lambda x, z: tris


def window_triangles(R, uw, radius):
    """tris_for of check_world on big meshes: the triangles of the rest cells within `radius` (>= the largest horizontal displacement)
    of the point, which hold every rest point that can be displaced onto it"""
    rc0 = float(rest_coords(R, uw)[0])

    def f(x, z):
        lo = lambda c: int(min(max(np.floor((c - radius - rc0) / uw) - 1, 0), R - 2))
        hi = lambda c: int(min(max(np.ceil((c + radius - rc0) / uw) + 1, 0), R - 2))
        ci, cj = np.meshgrid(np.arange(lo(x), hi(x) + 1), np.arange(lo(z), hi(z) + 1), indexing="ij")
        return grid_triangles(R, (ci.ravel(), cj.ravel()))
    return f


def check_world(out, xz, vert, norm, white, uw, tris_for, unique_exact=True):
    """Checks world-mode results out [n,8] of queries xz [n,2] against every displaced triangle tris_for(x, z) names:
      * always: the result is a point on the mesh, and its residual is its horizontal distance from the query;
      * where exactly one triangle holds the query (not on an edge): height within 1e-5 of the mesh's height scale, residual
        <= 1e-4 unit widths, normal and whitecap of that triangle.
    unique_exact=False (folded meshes, which can trap the walk in a fold next to a point they cover once): only the points it
    resolved (residual ~0) are held to their triangle.  Returns (unique points checked, points in folds, unique points missed)."""
    scale = float(np.abs(vert[:, 1]).max())
    wscale = max(1.0, float(np.abs(white).max()))
    plane = vert[:, [0, 2]]
    nuniq = nfold = nmissed = 0
    for k in range(len(xz)):
        r, x, z = out[k], float(xz[k, 0]), float(xz[k, 1])
        assert np.isfinite(r).all(), (k, xz[k], r)
        assert abs(r[7] - np.hypot(r[0] - x, r[2] - z)) <= 2e-6 * max(1.0, abs(x), abs(z)), (k, xz[k], r)
        assert on_mesh(r, vert, tris_for(float(r[0]), float(r[2])), 1e-4, 1e-4 * scale + 1e-6), (k, xz[k], r)
        tris = tris_for(x, z)
        t, w = containing(np.array([x]), np.array([z]), plane, tris, 1e-6)[0]
        ts = containing(np.array([x]), np.array([z]), plane, tris, -1e-6)[0][0]
        if len(t) == 1 and len(ts) == 1:   # exactly one displaced triangle holds the point, and not on an edge
            if not unique_exact and r[7] > 1e-4 * uw:
                nmissed += 1
                continue
            p, n, wh = _interp(tris[t[0]], w[0], vert, norm, white)
            assert abs(r[1] - p[1]) <= 1e-5 * scale, (k, xz[k], r, p)
            assert r[7] <= 1e-4 * uw, (k, xz[k], r)
            assert np.abs(r[3:6] - n).max() <= 1e-4 and abs(r[6] - wh) <= 1e-4 * wscale, (k, xz[k], r, n, wh)
            nuniq += 1
        elif len(t) > 1:
            nfold += 1
    return nuniq, nfold, nmissed
