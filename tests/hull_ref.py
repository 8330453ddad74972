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


def forces(x, d, u, tris, body, density, gravity, lin=0.0, quad=0.0):
    """row (Fx, Fy, Fz, area, tx, ty, tz) [7] of one body: instance vertices x [V, 3], depths d [V], water velocities u [V, 3]"""
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
