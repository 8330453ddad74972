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


# ---- edge point families (tests/test_surface_query_edges_cpu.py, _gpu.py) -------------------------------------------------------
def grid_line_points(R, uw, seed=0):
    """Rest-mode points on and beside the rest grid lines: every rest coordinate and its two float32 neighbours (3R line values), paired
    with a random in-range coordinate on the other axis, the same swapped, and line against line (a permutation of the line values, and
    each line value with itself: the vertices and the four corners).  [12R, 2] float32.  A coordinate below rc[0] or above rc[-1] is off
    the footprint (rest_reference: a NaN row); rc[0] and rc[-1] themselves are on it."""
    rc = rest_coords(R, uw)
    lines = np.concatenate([rc, np.nextafter(rc, f32(np.inf)), np.nextafter(rc, f32(-np.inf))]).astype(f32)
    rng = np.random.default_rng(seed)
    other = rng.uniform(float(rc[0]), float(rc[-1]), len(lines)).astype(f32)
    perm = lines[rng.permutation(len(lines))]
    return np.concatenate([np.stack([lines, other], -1), np.stack([other, lines], -1), np.stack([lines, perm], -1),
                           np.stack([lines, lines], -1)]).astype(f32)


def displaced_feature_points(vert, R):
    """World-mode points ON the displaced mesh's features, rounded to float32: the xz of every vertex, every edge midpoint along i and
    along j, every midpoint of a cell's diagonal (i, j+1)-(i+1, j).  [R^2 + 2R(R-1) + (R-1)^2, 2] float32."""
    g = vert[:, [0, 2]].astype(np.float64).reshape(R, R, 2)
    mid = lambda a, b: (0.5 * (a + b)).reshape(-1, 2)
    return np.concatenate([g.reshape(-1, 2), mid(g[:-1], g[1:]), mid(g[:, :-1], g[:, 1:]), mid(g[:-1, 1:], g[1:, :-1])]).astype(f32)


def off_footprint_ring(vert, R, uw, dist, n):
    """n world-mode points evenly along the square `dist` unit widths outside the bounding box of the displaced footprint."""
    x, z = vert[:, 0].astype(np.float64), vert[:, 2].astype(np.float64)
    x0, x1, z0, z1 = x.min() - dist * uw, x.max() + dist * uw, z.min() - dist * uw, z.max() + dist * uw
    s = (np.arange(n) + 0.5) / n * 4.0
    side, t = np.minimum(s.astype(int), 3), s - np.minimum(s.astype(int), 3)
    px = np.select([side == 0, side == 1, side == 2], [x0 + t * (x1 - x0), np.full(n, x1), x1 - t * (x1 - x0)], np.full(n, x0))
    pz = np.select([side == 0, side == 1, side == 2], [np.full(n, z0), z0 + t * (z1 - z0), np.full(n, z1)], z1 - t * (z1 - z0))
    return np.stack([px, pz], -1).astype(f32)


def border_distance(q, vert, R):
    """float64 distance of every point q [n, 2] to the closed polyline of the displaced border vertices."""
    g = vert[:, [0, 2]].astype(np.float64).reshape(R, R, 2)
    loop = np.concatenate([g[0, :-1], g[:-1, -1], g[-1, :0:-1], g[:0:-1, 0]])
    a, b = loop, np.roll(loop, -1, 0)
    q = np.asarray(q, np.float64)
    ab = b - a
    t = np.clip(((q[:, None] - a[None]) * ab[None]).sum(-1) / np.maximum((ab * ab).sum(-1), 1e-300)[None], 0.0, 1.0)
    return np.linalg.norm(a[None] + t[..., None] * ab[None] - q[:, None], axis=-1).min(1)


# ---- the brute force, vectorised over points: every triangle a point can lie on ---------------------------------------------------
def _window(px, pz, vert, R, uw):
    """Vertex ids [n, M, 3] (corner order of grid_triangles) of the triangles of every rest cell within dmax + 2 unit widths of each
    point, dmax the largest horizontal displacement of a finite vertex: a displaced triangle that holds the point has its rest cell
    there (all cells when the window covers the mesh), and their cells [n, M] (ci, cj)."""
    ok = np.isfinite(vert).all(-1)
    dmax = float(np.abs(vert[:, [0, 2]].astype(np.float64) - rest_plane(R, uw))[ok].max())
    k = int(np.ceil(dmax / uw)) + 2
    n = len(px)
    if 2 * k + 1 >= R - 1:
        ci, cj = np.meshgrid(np.arange(R - 1), np.arange(R - 1), indexing="ij")
        ci, cj = np.broadcast_to(ci.ravel(), (n, (R - 1) ** 2)), np.broadcast_to(cj.ravel(), (n, (R - 1) ** 2))
    else:
        rc0 = float(rest_coords(R, uw)[0])
        d = np.arange(-k, k + 1)
        di, dj = (a.ravel() for a in np.meshgrid(d, d, indexing="ij"))
        cell = lambda p: np.clip(np.nan_to_num(np.floor((np.asarray(p, np.float64) - rc0) / uw), nan=0.0, posinf=R, neginf=-R), -R, 2 * R)
        ci = cell(px)[:, None].astype(np.int64) + di[None]
        cj = cell(pz)[:, None].astype(np.int64) + dj[None]
    off = (ci < 0) | (ci > R - 2) | (cj < 0) | (cj > R - 2)
    c = np.where(off, 0, ci * R + cj)
    idx = np.concatenate([np.stack([c, c + 1, c + R], -1), np.stack([c + R, c + 1, c + R + 1], -1)], 1)
    idx[np.concatenate([off, off], 1)] = 0   # a cell off the mesh: the zero-area triangle (0, 0, 0), which holds no point
    return idx, np.concatenate([ci, ci], 1), np.concatenate([cj, cj], 1)


def _window_bary(px, pz, vert, idx):
    """barycentric weights [n, M, 3] of (px, pz) in the displaced triangles idx (NaN for a degenerate or non-finite triangle)"""
    P = vert[:, [0, 2]].astype(np.float64)[idx]
    a, v0, v1 = P[:, :, 0], P[:, :, 1] - P[:, :, 0], P[:, :, 2] - P[:, :, 0]
    with np.errstate(all="ignore"):
        d = v0[..., 0] * v1[..., 1] - v1[..., 0] * v0[..., 1]
        v2x, v2z = np.asarray(px, np.float64)[:, None] - a[..., 0], np.asarray(pz, np.float64)[:, None] - a[..., 1]
        wb = (v2x * v1[..., 1] - v1[..., 0] * v2z) / d
        wc = (v0[..., 0] * v2z - v2x * v0[..., 1]) / d
        return np.stack([1.0 - wb - wc, wb, wc], -1)


def on_mesh_rows(res, vert, R, uw, tol_xz, tol_y, chunk=1000):
    """on_mesh for every row of res [n, >= 3] at once -> bool [n]"""
    out = np.zeros(len(res), bool)
    for s in range(0, len(res), chunk):
        r = np.asarray(res[s:s + chunk], np.float64)
        idx, _, _ = _window(r[:, 0], r[:, 2], vert, R, uw)
        W = _window_bary(r[:, 0], r[:, 2], vert, idx)
        with np.errstate(all="ignore"):
            y = (W * vert[:, 1].astype(np.float64)[idx]).sum(-1)
            out[s:s + chunk] = ((np.nan_to_num(W.min(-1), nan=-1.0) >= -tol_xz) & (np.abs(y - r[:, 1:2]) <= tol_y)).any(1)
    return out


def world_reference(xz, ans_y, vert, norm, white, R, uw, tol=1e-6, vel=None, chunk=1000):
    """The float64 answer of world-mode queries xz [n, 2] on a mesh that does not fold there: of the displaced triangles that hold the
    point up to `tol` in barycentric weight (containing(..., tol)) the one whose interpolated height is nearest to ans_y [n] (the mesh is
    continuous across edges: on an edge or a vertex the neighbours agree).  -> (count [n] of such triangles, 0: off the footprint;
    local [n]: they all lie in one 2 x 2 block of cells, i.e. around one vertex or edge; ref [n, 7] (p, n, white); vref [n, 3] or None)"""
    n = len(xz)
    count, local = np.zeros(n, np.int64), np.zeros(n, bool)
    ref, vref = np.full((n, 7), np.nan), (None if vel is None else np.full((n, 3), np.nan))
    V, N, Wh = vert.astype(np.float64), norm.astype(np.float64), white.astype(np.float64)
    for s in range(0, n, chunk):
        x, z = xz[s:s + chunk, 0].astype(np.float64), xz[s:s + chunk, 1].astype(np.float64)
        idx, ci, cj = _window(x, z, vert, R, uw)
        W = _window_bary(x, z, vert, idx)
        inside = np.nan_to_num(W.min(-1), nan=-1.0) >= -tol
        m = len(x)
        count[s:s + m] = inside.sum(1)
        big = np.iinfo(np.int64).max
        span = lambda c: np.where(inside, c, -1).max(1) - np.where(inside, c, big).min(1)
        local[s:s + m] = inside.any(1) & (span(ci) <= 1) & (span(cj) <= 1)
        with np.errstate(all="ignore"):
            y = (W * V[:, 1][idx]).sum(-1)
        pick = np.where(inside, np.abs(y - np.asarray(ans_y[s:s + m], np.float64)[:, None]), np.inf).argmin(1)
        rows = np.arange(m)
        t, w = idx[rows, pick], W[rows, pick]
        ref[s:s + m, :3] = (w[..., None] * V[t]).sum(1)
        nn = (w[..., None] * N[t]).sum(1)
        ref[s:s + m, 3:6] = nn / np.linalg.norm(nn, axis=-1, keepdims=True)
        ref[s:s + m, 6] = (w * Wh[t]).sum(1)
        if vel is not None:
            vref[s:s + m] = (w[..., None] * vel.astype(np.float64)[t]).sum(1)
        ref[s:s + m][~inside.any(1)] = np.nan
    return count, local, ref, vref
