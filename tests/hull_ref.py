"""numpy float64 reference of mw_ocean_hull_forces (include/mistral_water.h, csrc/hull_forces.h) and test hulls.

The reference restates the maths independently of the kernels: the pose transform, the clip of each triangle at d = 0, the closed-form
pressure integrals, the drag terms, and -- for the Archimedes checks -- the volume and centroid of a closed mesh below a plane, from
signed tetrahedra whose common apex lies ON the plane: the waterline cap that closes the submerged part then spans tetrahedra of zero
volume, so the clipped triangles alone give the volume and its centroid."""
import numpy as np


def rotation(q):
    """rotation matrices [n, 3, 3] of quaternions q [n, 4] = (x, y, z, w), normalised first"""
    q = np.asarray(q, np.float64).reshape(-1, 4)
    q = q / np.linalg.norm(q, axis=1, keepdims=True)
    x, y, z, w = q.T
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], 1)


def transform(bodies, hull):
    """instance vertices x [n, V, 3] = p + R(q) h of bodies [n, 16] and hull [V, 3]"""
    b = np.asarray(bodies, np.float64).reshape(-1, 16)
    return b[:, None, 0:3] + np.einsum("nij,vj->nvi", rotation(b[:, 4:8]), np.asarray(hull, np.float64))


def clip(x, d, u):
    """the submerged sub-triangles of one triangle (corners x [3, 3], depths d [3], water velocities u [3, 3]) -> list of (x, d, u);
    wet means d > 0, cut points interpolate linearly along the edge, winding kept"""
    wet = d > 0
    n = int(wet.sum())
    if n == 0:
        return []
    if n == 3:
        return [(x, d, u)]
    f = int(np.nonzero(wet)[0][0]) if n == 1 else int(np.nonzero(~wet)[0][0])
    a, b, c = f, (f + 1) % 3, (f + 2) % 3

    def cut(w, dry):
        t = d[w] / (d[w] - d[dry])
        return x[w] + t * (x[dry] - x[w]), 0.0, u[w] + t * (u[dry] - u[w])

    def tri(*pts):
        return np.array([p[0] for p in pts]), np.array([p[1] for p in pts]), np.array([p[2] for p in pts])

    A, B, Cc = (x[a], d[a], u[a]), (x[b], d[b], u[b]), (x[c], d[c], u[c])
    if n == 1:
        return [tri(A, cut(a, b), cut(a, c))]
    ab, ca = cut(b, a), cut(c, a)
    return [tri(ab, B, Cc), tri(ab, Cc, ca)]


def subtriangle(x, d, u, p, v, w, rho_g, lin, quad):
    """(F[3], area, tau[3]) of one submerged sub-triangle about p"""
    S = 0.5 * np.cross(x[1] - x[0], x[2] - x[0])
    r = x - p
    D = d.sum()
    F = -rho_g * D / 3 * S
    tau = -rho_g / 12 * np.cross((d[:, None] * r).sum(0) + D * r.sum(0), S)
    A = float(np.linalg.norm(S))
    if lin or quad:
        rc = r.mean(0)
        vr = v + np.cross(w, rc) - u.mean(0)
        Fd = -lin * A * vr
        if A > 0:
            n = S / A
            vn = float(vr @ n)
            if vn > 0:
                Fd = Fd - quad * A * vn * vn * n
        F = F + Fd
        tau = tau + np.cross(rc, Fd)
    return F, A, tau


def forces(x, d, u, tris, body, density, gravity, lin=0.0, quad=0.0, terms=False):
    """row (Fx, Fy, Fz, area, tx, ty, tz) [7] of one body: instance vertices x [V, 3], depths d [V], water velocities u [V, 3].
    terms: (row, per-triangle terms [T, 7]) from forces_terms, the same maths over all triangles at once (quick on large hulls); the row
    is the float64 sum of the terms."""
    if terms:
        per = forces_terms(x, d, u, tris, body, density, gravity, lin, quad)
        return per.sum(0), per
    body = np.asarray(body, np.float64)
    p, v, w = body[0:3], body[8:11], body[12:15]
    x, d, u = np.asarray(x, np.float64), np.asarray(d, np.float64), np.asarray(u, np.float64)
    row = np.zeros(7)
    for t in np.asarray(tris):
        for sx, sd, su in clip(x[t], d[t], u[t]):
            F, A, tau = subtriangle(sx, sd, su, p, v, w, density * gravity, lin, quad)
            row[0:3] += F
            row[3] += A
            row[4:7] += tau
    return row


def _subtriangles(x, d, u, p, v, w, rho_g, lin, quad):
    """subtriangle() over m sub-triangles at once: x [m, 3, 3], d [m, 3], u [m, 3, 3] -> terms [m, 7]"""
    S = 0.5 * np.cross(x[:, 1] - x[:, 0], x[:, 2] - x[:, 0])
    r = x - p
    D = d.sum(1)
    F = -rho_g * (D / 3)[:, None] * S
    tau = -rho_g / 12 * np.cross((d[:, :, None] * r).sum(1) + D[:, None] * r.sum(1), S)
    A = np.linalg.norm(S, axis=1)
    if lin or quad:
        rc = r.mean(1)
        vr = v + np.cross(w, rc) - u.mean(1)
        Fd = -lin * A[:, None] * vr
        with np.errstate(invalid="ignore", divide="ignore"):
            n = np.where(A[:, None] > 0, S / A[:, None], 0.0)
        vn = np.einsum("ij,ij->i", vr, n)
        push = (A > 0) & (vn > 0)
        Fd = Fd - np.where(push, quad * A * vn * vn, 0.0)[:, None] * n
        F = F + Fd
        tau = tau + np.cross(rc, Fd)
    return np.concatenate([F, A[:, None], tau], 1)


def forces_terms(x, d, u, tris, body, density, gravity, lin=0.0, quad=0.0):
    """the terms (Fx, Fy, Fz, area, tx, ty, tz) [T, 7] each triangle adds to forces()'s row: the clip and the integrals of clip() and
    subtriangle() written over all triangles at once, float64 throughout"""
    body = np.asarray(body, np.float64)
    p, v, w = body[0:3], body[8:11], body[12:15]
    x, d, u = np.asarray(x, np.float64), np.asarray(d, np.float64), np.asarray(u, np.float64)
    t = np.asarray(tris)
    X, Dp, U = x[t], d[t], u[t]
    wet = Dp > 0
    n = wet.sum(1)
    out = np.zeros((len(t), 7))
    args = (p, v, w, density * gravity, lin, quad)
    full = np.nonzero(n == 3)[0]
    out[full] = _subtriangles(X[full], Dp[full], U[full], *args)

    def rotated(sel, first):  # corners of triangles sel in the order first, first + 1, first + 2 (cyclic: the winding stays)
        o = (first[:, None] + np.arange(3)) % 3
        k = sel[:, None]
        return X[k, o], Dp[k, o], U[k, o]

    def cut(xw, dw, uw, xd, dd, ud):  # from a wet corner to a dry one, as clip()'s cut
        s = (dw / (dw - dd))[:, None]
        return xw + s * (xd - xw), uw + s * (ud - uw)

    one = np.nonzero(n == 1)[0]
    if len(one):
        x3, d3, u3 = rotated(one, wet[one].argmax(1))
        xb, ub = cut(x3[:, 0], d3[:, 0], u3[:, 0], x3[:, 1], d3[:, 1], u3[:, 1])
        xc, uc = cut(x3[:, 0], d3[:, 0], u3[:, 0], x3[:, 2], d3[:, 2], u3[:, 2])
        z = np.zeros(len(one))
        out[one] = _subtriangles(np.stack([x3[:, 0], xb, xc], 1), np.stack([d3[:, 0], z, z], 1), np.stack([u3[:, 0], ub, uc], 1), *args)
    two = np.nonzero(n == 2)[0]
    if len(two):
        x3, d3, u3 = rotated(two, (~wet[two]).argmax(1))
        xab, uab = cut(x3[:, 1], d3[:, 1], u3[:, 1], x3[:, 0], d3[:, 0], u3[:, 0])
        xca, uca = cut(x3[:, 2], d3[:, 2], u3[:, 2], x3[:, 0], d3[:, 0], u3[:, 0])
        z = np.zeros(len(two))
        out[two] = (_subtriangles(np.stack([xab, x3[:, 1], x3[:, 2]], 1), np.stack([z, d3[:, 1], d3[:, 2]], 1),
                                  np.stack([uab, u3[:, 1], u3[:, 2]], 1), *args) +
                    _subtriangles(np.stack([xab, x3[:, 2], xca], 1), np.stack([z, d3[:, 2], z], 1), np.stack([uab, u3[:, 2], uca], 1), *args))
    return out


def term_scales(per):
    """(S_F, S_tau) of per-triangle terms [T, 7]: the sums over the triangles of |F_t| and |tau_t| -- the scale a summation error or
    a lost triangle is measured against; unlike the whole hull's buoyancy it exists for an open mesh"""
    return float(np.linalg.norm(per[:, 0:3], axis=1).sum()), float(np.linalg.norm(per[:, 4:7], axis=1).sum())


def submerged(x, tris, level=0.0):
    """(volume, centroid[3]) of the part of the closed mesh x [V, 3] (outward winding) below the plane y = level"""
    x = np.asarray(x, np.float64)
    d = level - x[:, 1]
    q = np.array([x[:, 0].mean(), level, x[:, 2].mean()])  # apex on the plane: the cap's tetrahedra are flat
    vol, mom = 0.0, np.zeros(3)
    for t in np.asarray(tris):
        for sx, _, _ in clip(x[t], d[t], np.zeros((3, 3))):
            a, b, c = sx - q
            vt = float(a @ np.cross(b, c)) / 6
            vol += vt
            mom += vt * (sx.sum(0) + q) / 4
    return vol, mom / vol if vol else np.zeros(3)


def volume(x, tris):
    """volume of the closed mesh x [V, 3]"""
    x = np.asarray(x, np.float64)
    t = np.asarray(tris)
    return float(np.einsum("ij,ij->i", x[t[:, 0]], np.cross(x[t[:, 1]], x[t[:, 2]])).sum() / 6)


# ---- test hulls (outward winding: (b - a) x (c - a) points out) ---------------------------------------------------------------
def box(w, h, l):
    """axis-aligned box centred at the origin, extent w (x) h (y) l (z): 8 vertices, 12 triangles"""
    v = np.array([[sx * w / 2, sy * h / 2, sz * l / 2] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)], np.float32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tris = []
    for a, b, c, dd in quads:
        tris += [(a, b, c), (a, c, dd)]
    return v, _outward(v, np.array(tris, np.int32))


def icosphere(radius=1.0, subdiv=2):
    """icosphere: 12 vertices and 20 triangles, each subdivision x4 triangles (2 levels: 162 vertices, 320 triangles)"""
    t = (1 + 5 ** 0.5) / 2
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    x = (np.array(v) * radius).astype(np.float32)
    return x, _outward(x, np.array(f, np.int32))


def grid_hull(nx, nz, w, l, depth):
    """a closed barge of about 4 nx nz triangles: a w x l bottom at y = -depth and a deck at y = 0, each split into nx x nz cells,
    and four walls between them; outward winding"""
    xs, zs = np.linspace(-w / 2, w / 2, nx + 1), np.linspace(-l / 2, l / 2, nz + 1)
    verts, tris = [], []

    def sheet(P):  # P [a, b, 3] grid of points -> triangles, winding as given
        base = len(verts)
        A, B = P.shape[:2]
        verts.extend(P.reshape(-1, 3))
        for i in range(A - 1):
            for j in range(B - 1):
                c = base + i * B + j
                tris.extend([(c, c + 1, c + B + 1), (c, c + B + 1, c + B)])
    X, Z = np.meshgrid(xs, zs, indexing="ij")
    sheet(np.stack([X, np.full_like(X, -depth), Z], -1))
    sheet(np.stack([X, np.zeros_like(X), Z], -1))
    ys = np.linspace(-depth, 0, 3)
    for fixed, axis in ((-w / 2, 0), (w / 2, 0), (-l / 2, 2), (l / 2, 2)):
        other = zs if axis == 0 else xs
        O, Y = np.meshgrid(other, ys, indexing="ij")
        P = np.stack([np.full_like(O, fixed), Y, O], -1) if axis == 0 else np.stack([O, Y, np.full_like(O, fixed)], -1)
        sheet(P)
    x = np.array(verts, np.float32)
    t = np.array(tris, np.int32)
    # per-triangle outward test against the box centre (a convex hull: every face normal points away from the centre)
    c = np.array([0, -depth / 2, 0])
    xx = x.astype(np.float64)
    n = np.cross(xx[t[:, 1]] - xx[t[:, 0]], xx[t[:, 2]] - xx[t[:, 0]])
    flip = np.einsum("ij,ij->i", n, xx[t].mean(1) - c) < 0
    t[flip] = t[flip][:, [0, 2, 1]]
    return x, t


# ---- the edge hulls: triangle and vertex counts at the chunk and reduce-lap edges of the kernels' summation (csrc/hull_forces.h) ----
SENTINEL_AT = (0, 255, 256, 16383, 16384)  # and ntris - 1: first and last lane of a chunk, last chunk of a lap and first of the next
EDGE_W, EDGE_DEPTH = 6.0, 1.5


def edge_base(ntris):
    """(nx, nz) of the barge edge_hull cuts: 6 x 8 cells (222 vertices, 304 triangles: fewer than 255 vertices, so the triangles set the
    chunk count) up to 257 triangles, 64^2 (9230 vertices, 17 408 triangles) up to 16 385, 91^2 (18 032, 34 580) above"""
    return (6, 8) if ntris <= 257 else (64, 64) if ntris <= 16385 else (91, 91)


def sentinel_slots(ntris):
    return sorted({k for k in SENTINEL_AT + (ntris - 1,) if 0 <= k < ntris})


def edge_hull(ntris, nverts=None, cells=None, seed=0):
    """(hull_xyz, triangles) of grid_hull(nx, nz, 6, 6, 1.5) (cells = (nx, nz), default edge_base(ntris)) cut to its first ntris triangles
    -- an open mesh: the bottom sheet comes first -- with unreferenced vertices inside the bounding box appended up to nverts, and the
    triangles at sentinel_slots(ntris) replaced by sentinels: three corners of the bottom sheet wound outward (downward), area 18
    against a cell triangle's 0.0044 at 64^2, so that a sum that loses one of those slots is wrong in its first digit."""
    nx, nz = cells or edge_base(ntris)
    x, t = grid_hull(nx, nz, EDGE_W, EDGE_W, EDGE_DEPTH)
    assert ntris <= len(t) and (nverts is None or nverts >= len(x)), (ntris, len(t), nverts, len(x))
    t = t[:ntris].copy()
    corners = [0, nz, nx * (nz + 1) + nz, nx * (nz + 1)]  # around the bottom sheet
    xx = x.astype(np.float64)
    for n, k in enumerate(sentinel_slots(ntris)):
        a, b, c = (corners[(n + j) % 4] for j in range(3))
        if np.cross(xx[b] - xx[a], xx[c] - xx[a])[1] > 0:  # outward is down
            b, c = c, b
        t[k] = (a, b, c)
    if nverts is not None and nverts > len(x):
        rng = np.random.default_rng(seed)
        m = nverts - len(x)
        extra = np.stack([rng.uniform(-EDGE_W / 2, EDGE_W / 2, m), rng.uniform(-EDGE_DEPTH, 0, m), rng.uniform(-EDGE_W / 2, EDGE_W / 2, m)], 1)
        x = np.concatenate([x, extra.astype(np.float32)])
    return np.ascontiguousarray(x), np.ascontiguousarray(t)


def bottom_corners():
    """the four corners of edge_hull's bottom sheet in body space [4, 3] (the sentinels' vertices)"""
    h = EDGE_W / 2
    return np.array([[-h, -EDGE_DEPTH, -h], [-h, -EDGE_DEPTH, h], [h, -EDGE_DEPTH, h], [h, -EDGE_DEPTH, -h]], np.float32)


def upright_quaternions(n, rng, tilt_deg=15.0):
    """n quaternions (x, y, z, w): any heading about y, then a tilt of at most tilt_deg about a horizontal axis"""
    yaw = rng.uniform(0, 2 * np.pi, n)
    tilt = np.deg2rad(rng.uniform(-tilt_deg, tilt_deg, n))
    ax = rng.uniform(0, 2 * np.pi, n)
    qt = np.stack([np.cos(ax) * np.sin(tilt / 2), np.zeros(n), np.sin(ax) * np.sin(tilt / 2), np.cos(tilt / 2)], 1)
    qy = np.stack([np.zeros(n), np.sin(yaw / 2), np.zeros(n), np.cos(yaw / 2)], 1)
    # Hamilton product qt (x) qy: heading first, then the tilt
    v1, w1, v2, w2 = qt[:, :3], qt[:, 3:], qy[:, :3], qy[:, 3:]
    q = np.concatenate([w1 * v2 + w2 * v1 + np.cross(v1, v2), w1 * w2 - (v1 * v2).sum(1, keepdims=True)], 1)
    return q.astype(np.float32)


def afloat_poses(n, rng, span, eta, tile_shift=None):
    """n poses (p [n, 3], q [n, 4]) that keep edge_hull's bottom sheet wet: p.xz within +-span, upright within +-15 degrees, p.y within
    [-0.4, 0.2] of the water under p, and of such candidates the first n whose four bottom corners all lie at least 0.1 under the water
    above them.  eta(xz [m, 2]) -> water height [m].  A sentinel spans three of those corners, so it is wet at every corner: a dry body
    would test nothing.  tile_shift (dx, dz): added to the last pose's p.xz before anything is looked up (a body in another tile)."""
    m = 64 * n
    p = np.stack([rng.uniform(-span, span, m), np.zeros(m), rng.uniform(-span, span, m)], 1)
    if tile_shift is not None:
        p[n - 1::n, 0] += tile_shift[0]
        p[n - 1::n, 2] += tile_shift[1]
    p = p.astype(np.float32)
    q = upright_quaternions(m, rng)
    p[:, 1] = eta(p[:, [0, 2]]) + rng.uniform(-0.4, 0.2, m)
    b = np.zeros((m, 16), np.float32)
    b[:, 0:3], b[:, 4:8] = p, q
    c = transform(b, bottom_corners())  # [m, 4, 3]
    depth = eta(c.reshape(-1, 3)[:, [0, 2]].astype(np.float32)).reshape(m, 4) - c[:, :, 1]
    ok = (depth > 0.1).all(1)
    # slot k of the result comes from the candidates k, k + n, ...: the shifted pose stays the last one
    pick = []
    for k in range(n):
        cand = np.nonzero(ok[k::n])[0]
        assert len(cand), "no candidate pose keeps the bottom sheet wet"
        pick.append(k + n * cand[0])
    return p[pick], q[pick]


def _outward(x, tris):
    """flip every triangle of a convex mesh around its centroid so that (b - a) x (c - a) points away from it"""
    xx = np.asarray(x, np.float64)
    c = xx.mean(0)
    n = np.cross(xx[tris[:, 1]] - xx[tris[:, 0]], xx[tris[:, 2]] - xx[tris[:, 0]])
    flip = np.einsum("ij,ij->i", n, xx[tris].mean(1) - c) < 0
    tris = tris.copy()
    tris[flip] = tris[flip][:, [0, 2, 1]]
    return tris


def random_quaternions(n, rng):
    q = rng.standard_normal((n, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
