"""Which fault a surface service reports when a call has two (csrc/surface_services.inc), pinned row by row: the status and the
mw_last_error() text of every entry point of the services that read the displaced surface, recorded on the commit before their host
path was rewritten and asserted as literals since.

Every row is one call through the C ABI on one of five small handles (64^2 FFTMesh with a frame; the same with no frame; a periodic one
whose spectrum was set again after its frame, so the frame is behind; OceanRenderer resolution 8; a batch of two tiles) or on NULL, with
the 8-vertex box hull, two bodies and lines_per_body = 2.  No row launches a kernel: a row fails, or is an empty call.  The orders the
rows pin:

* a device form tests alignment before it looks at the handle (NULL handle + misaligned pointer: alignment), and only for a call that is
  not empty; a fleet refuses draught before alignment and before everything else but the NULL handle;
* query_prepare: NULL handle, n, NULL array, mode, iterations, the one-launch limit, then the batched handle and the frame rules;
* prepare runs to its end, state rules included, before the empty-call return (n == 0 with no frame: MW_ESTATE); the host-only checks
  run after it (n == 0 with a bad triangle index: MW_OK);
* stepping checks its own arguments before the hull's, the moored call its own before those; triangles before mass rows, mass row b
  before body b's slots (or wrench row), body by body;
* mw_ocean_raycast_tiled refuses an OceanRenderer handle before it looks at reach; the column's "no column set" and frame-behind rules
  come after every argument check.

After every row the caller's host arrays are what they were.  MW_OK rows assert the status alone (mw_last_error() keeps the last
failure's text)."""
import ctypes as C

import numpy as np
import pytest

import hull_ref as H
import workloads

pytestmark = pytest.mark.gpu
RHO, G = 1000.0, 9.81
NB, K = 2, 2
# byte offsets of the device arrays in one buffer (each 256-byte aligned); vel holds the 64^2 x 3 floats a velocity call writes
OFF = dict(hull=0, tris=256, bodies=512, mass=768, lines=1024, out=1280, ten=1536, wrench=1792, xz=2048, xyz=2304, rays=2560, qout=2816,
           hit=3328, vel=4096)
DEV_BYTES = 4096 + 64 * 64 * 3 * 4


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


class Ctx:
    """the five handles, the host arrays of a valid call, their variants with one bad row, and the device buffer"""

    def __init__(self, mw, stack):
        import torch
        self.mw, self.L = mw, mw.lib()
        p = workloads.fftmesh_params(64, choppiness=1.0)

        def fft():
            return stack.enter_context(mw.Ocean(resolution=p.N, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y),
                                                amplitude=p.amplitude, choppiness=p.choppiness, gravity=p.gravity, seed=3, device=0))

        def renderer(**kw):
            return stack.enter_context(mw.Ocean(resolution=8, unit_width=1.0, length=27.155, wind=(14.45, 12.0), amplitude=0.41,
                                                choppiness=1.5, mult=1.5, seed=1, semantics=mw.MW_SEM_OCEANRENDERER, device=0, **kw))
        fm, nf, per, rend, batch = fft(), fft(), fft(), renderer(), renderer(ntiles=2)
        fm.evaluate(1.7)
        per.evaluate(1.7)
        per.set_periodic(True)
        per.set_spectrum(*per.get_spectrum())  # the frame is now behind the spectrum
        rend.generate_texture(0.3)
        batch.generate_texture(0.3)
        self.handles = dict(fm=fm, nf=nf, per=per, rend=rend, batch=batch)
        x, t = H.box(1.5, 1.0, 2.0)
        m, c, inertia = mw.hull_mass_properties(x, t, 600.0)
        mass = np.repeat(mw.pack_mass(m, inertia), NB, 0)
        lines = mw.pack_lines(NB, K, anchor=[[[0.0, -5.0, 0.0]] * K] * NB, rest_length=1.0, stiffness=100.0)
        self.host = dict(
            hull=np.asarray(x - c, np.float32), tris=np.ascontiguousarray(t, np.int32),
            bodies=mw.pack_bodies([[0.0, 0.0, 0.0], [3.0, 0.0, 1.0]]), mass=mass, lines=lines, out=np.full((NB, 8), 7.0, np.float32),
            ten=np.full((NB, K), 7.0, np.float32), wrench=np.zeros((NB, 8), np.float32), xz=np.zeros((4, 2), np.float32),
            xyz=np.zeros((4, 4), np.float32), rays=np.zeros((4, 8), np.float32), qout=np.full((4, 16), 7.0, np.float32),
            hit=np.full((4, 4), 7, np.int32), vel=np.full((64 * 64, 3), 7.0, np.float32),
            coeffs=np.array([RHO, G, 0, 0, 1], np.float32), table=np.array([[0, 8, 0, 12, NB]], np.int32))
        assert self.host["hull"].shape == (8, 3) and self.host["tris"].shape == (12, 3) and lines.size == NB * K * 12

        def edit(name, index, value):
            a = self.host[name].copy()
            a.reshape(-1)[index] = value
            return a
        self.bad = dict(
            tris=edit("tris", 0, 8), mass0=edit("mass", 0, -1.0), mass1=edit("mass", 8, -1.0), coeffs=edit("coeffs", 2, np.nan),
            slot00=edit("lines", 0, np.nan), slot01=edit("lines", 12, np.nan), slot10=edit("lines", 24, np.nan),
            wrench0=edit("wrench", 0, np.nan), table_nverts=edit("table", 1, 2), table_empty=edit("table", 4, 0))
        self.bad["mass01"] = np.concatenate([self.bad["mass0"][:1], self.bad["mass1"][1:]])
        self.snapshot = {k: v.copy() for k, v in self.host.items()}
        self.buf = torch.zeros(DEV_BYTES // 4, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        self.base = self.buf.data_ptr()
        assert self.base % 256 == 0

    def untouched(self):
        return all(np.array_equal(v.view(np.uint8), self.snapshot[k].view(np.uint8)) for k, v in self.host.items())


class Call:
    """one call: the pointers of the host or the device form, with the row's overrides.  null: names passed as NULL; mis: a device array
    passed 2 bytes off; a keyword named like an array (tris=...) names the entry of Ctx.bad the host form passes in its place."""

    def __init__(self, cx, h, dev, kw):
        self.cx, self.h, self.dev, self.kw = cx, h, dev, dict(kw)
        self.null, self.mis = self.kw.pop("null", ()), self.kw.pop("mis", None)

    def fn(self, name):
        return getattr(self.cx.L, "mw_ocean_" + name + ("_device" if self.dev else ""))

    def ptr(self, name, host_only=False):
        if name in self.null:
            return None
        if self.dev and not host_only:
            return C.c_void_p(self.cx.base + OFF[name] + (2 if name == self.mis else 0))
        return _p(self.cx.bad[self.kw[name]] if name in self.kw else self.cx.host[name])

    def get(self, name, default):
        return self.kw.get(name, default)


def _query(c, name="query_surface", pts="xz"):
    return c.fn(name)(c.h, c.get("frame", -1), c.get("mode", 1), c.ptr(pts), c.get("n", 4), c.get("it", 0), c.ptr("qout"))


def query_surface(c):
    return _query(c)


def query_velocity(c):
    return _query(c, "query_velocity")


def query_column(c):
    return _query(c, "query_column", "xyz")


def raycast(c):
    return c.fn("raycast")(c.h, c.get("frame", -1), c.ptr("rays"), c.get("n", 4), c.ptr("qout"), c.ptr("hit"))


def raycast_tiled(c):
    return c.fn("raycast_tiled")(c.h, c.get("frame", -1), c.ptr("rays"), c.get("n", 4), c.get("reach", 4), c.ptr("qout"), c.ptr("hit"))


def velocity(c):
    return c.fn("velocity")(c.h, c.get("frame", -1), c.ptr("vel"))


def hull_forces(c):
    return c.fn("hull_forces")(c.h, c.get("frame", -1), c.ptr("hull"), c.get("nverts", 8), c.ptr("tris"), 12, c.ptr("bodies"), c.get("nb", NB),
                               c.ptr("coeffs", True), c.get("it", 0), c.ptr("out"))


def step_bodies(c):
    return c.fn("step_bodies")(c.h, c.get("frame", -1), c.ptr("hull"), c.get("nverts", 8), c.ptr("tris"), 12, c.ptr("bodies"), c.ptr("mass"),
                               c.get("nb", NB), c.ptr("coeffs", True), C.c_float(c.get("dt", 0.1)), c.get("sub", 1), c.get("it", 0), c.ptr("out"))


def step_moored(c):
    return c.fn("step_moored")(c.h, c.get("frame", -1), c.ptr("hull"), c.get("nverts", 8), c.ptr("tris"), 12, c.ptr("bodies"), c.ptr("mass"),
                               c.ptr("lines"), c.get("K", K), c.get("nb", NB), c.ptr("coeffs", True), C.c_float(c.get("dt", 0.1)),
                               c.get("sub", 1), c.get("it", 0), c.ptr("out"), c.ptr("ten"))


def fleet_forces(c):
    return c.fn("fleet_forces")(c.h, c.get("frame", -1), c.ptr("hull"), 8, c.ptr("tris"), 12, c.ptr("table", True), c.get("nhulls", 1),
                                c.ptr("bodies"), c.get("tb", NB), c.ptr("coeffs", True), c.get("it", 0), c.ptr("out"))


def step_fleet(c):
    return c.fn("step_fleet")(c.h, c.get("frame", -1), c.ptr("hull"), 8, c.ptr("tris"), 12, c.ptr("table", True), c.get("nhulls", 1),
                              c.ptr("bodies"), c.ptr("mass"), c.ptr("wrench"), c.get("tb", NB), c.ptr("coeffs", True),
                              C.c_float(c.get("dt", 0.1)), c.get("sub", 1), c.get("it", 0), c.ptr("out"))


EINVAL, ESTATE, OK = 1, 6, 0
BATCHED = "a batched handle (mw_ocean_create_batch) has no single surface"
NO_FRAME = "no frame yet (mw_ocean_evaluate / mw_ocean_update first)"
ONE_FRAME = "FFTMesh handles keep one frame (frame = -1)"
BEHIND_VEL = ("the spectrum or phase changed after the latest frame: the surface and the velocity would belong to different instants "
              "(make a frame first)")
BEHIND_COL = ("the spectrum or phase changed after the latest frame: the surface and the layers would belong to different instants "
              "(make a frame first)")
NO_COLUMN = "no column set (mw_ocean_set_column first)"
NO_COLUMN_HANDLE = "an OceanRenderer or batched handle has no column (its mesh samples clamp-addressed textures): FFTMesh handles only"
NOT_TILING = "an OceanRenderer mesh does not tile (mw_ocean_set_periodic)"
REACH = "reach must be in [0, MW_RC_MAX_REACH]"
TRIANGLE = "triangle index outside [0, nverts)"
SUBSTEPS = "substeps must be in [1, 64]"
LINES = "lines_per_body must be in [1, MW_MOORING_MAX_LINES]"
DRAUGHT = ("fleets do not read the water column yet: the handle has draught on (mw_ocean_set_draught(o, 0) first, or "
           "mw_ocean_hull_forces / mw_ocean_step_bodies per hull)")
ALIGN_Q = "d_xz must be 8-byte and d_out 16-byte aligned"
ALIGN_HULL = "d_hull_xyz and d_triangles must be 4-byte, d_bodies and d_out 16-byte aligned"
ALIGN_BODIES = "d_hull_xyz and d_triangles must be 4-byte, d_bodies, d_mass and d_out 16-byte aligned"
ALIGN_MOORED = "d_hull_xyz, d_triangles and d_tension must be 4-byte, d_bodies, d_mass, d_lines and d_out 16-byte aligned"
ALIGN_FLEET = "d_hull_xyz and d_triangles must be 4-byte, d_bodies, d_mass, d_wrench and d_out 16-byte aligned"
ALIGN_RAY = "d_rays and d_out must be 16-byte and d_hit 8-byte aligned"


def mass_row(b):
    return f"the mass row of body {b} is invalid (m <= 0 or not finite, or I_b not positive definite)"


def slot(k, b):
    return f"slot {k} of body {b} is invalid (a non-finite float, or L0, k or c negative)"


# (service, handle, device form, overrides, status, message after "<entry point>: ").  Handle-level switches of a row: draught=True turns
# draught on for the call, column=True sets a three-layer column for it; both are undone after the row.
ROWS = [
    # ---- the device forms: alignment before the handle ----
    (query_surface, None, True, dict(mis="xz"), EINVAL, ALIGN_Q),
    (query_velocity, None, True, dict(mis="qout"), EINVAL, ALIGN_Q),
    (query_column, None, True, dict(mis="xyz"), EINVAL, "d_xyz_ and d_out must be 16-byte aligned"),
    (raycast, None, True, dict(mis="hit"), EINVAL, ALIGN_RAY),
    (raycast_tiled, None, True, dict(mis="hit"), EINVAL, "d_rays, d_out and d_hit must be 16-byte aligned"),
    (hull_forces, None, True, dict(mis="tris"), EINVAL, ALIGN_HULL),
    (step_bodies, None, True, dict(mis="mass"), EINVAL, ALIGN_BODIES),
    (step_moored, None, True, dict(mis="ten"), EINVAL, ALIGN_MOORED),
    (fleet_forces, None, True, dict(mis="bodies"), EINVAL, ALIGN_FLEET),
    (step_fleet, None, True, dict(mis="wrench"), EINVAL, ALIGN_FLEET),
    (query_surface, None, True, dict(mis="xz", n=0), EINVAL, "NULL handle"),  # an empty call has no alignment to test
    (query_surface, "batch", True, dict(mis="qout", mode=7), EINVAL, ALIGN_Q),
    (raycast, "per", True, dict(mis="rays", n=-1), EINVAL, "n < 0"),
    (raycast, "per", True, dict(mis="rays"), EINVAL, ALIGN_RAY),
    (hull_forces, "fm", True, dict(mis="out", nb=-1), EINVAL, "nbodies < 0"),
    (step_bodies, "fm", True, dict(mis="bodies", sub=0), EINVAL, ALIGN_BODIES),
    (step_moored, "fm", True, dict(mis="lines", K=0), EINVAL, ALIGN_MOORED),
    (step_fleet, "fm", True, dict(mis="mass", draught=True), ESTATE, DRAUGHT),
    (fleet_forces, "fm", True, dict(mis="out", nhulls=0), EINVAL, ALIGN_FLEET),
    (query_column, "nf", True, dict(n=0), ESTATE, NO_FRAME),
    (raycast_tiled, "rend", True, dict(reach=-1), ESTATE, NOT_TILING),
    (query_velocity, "per", True, dict(n=0), ESTATE, BEHIND_VEL),
    # ---- query_prepare's order ----
    (query_surface, None, False, dict(n=-1), EINVAL, "NULL handle"),
    (query_surface, "batch", False, dict(n=-1), EINVAL, "n < 0"),
    (query_surface, "batch", False, dict(null=("qout",)), EINVAL, "NULL array"),
    (query_surface, "batch", False, dict(mode=7), EINVAL, "mode must be MW_QUERY_REST or MW_QUERY_WORLD"),
    (query_surface, "batch", False, dict(it=65), EINVAL, "iterations must be in [0,64]"),
    (query_surface, "batch", False, dict(n=2 ** 32), EINVAL, "n > 2^32 - 256 (one launch)"),
    (query_surface, "batch", False, dict(frame=5), EINVAL, BATCHED),
    (query_surface, "nf", False, dict(frame=0), EINVAL, ONE_FRAME),
    (query_surface, "nf", False, dict(n=0), ESTATE, NO_FRAME),
    (query_surface, "fm", False, dict(n=0, null=("xz", "qout")), OK, None),
    (query_surface, "rend", False, dict(frame=7), EINVAL, "frame out of range (-1, or a frame of the latest steps call)"),
    # ---- velocity and the velocity query ----
    (velocity, None, False, dict(null=("vel",)), EINVAL, "NULL handle"),
    (velocity, "batch", True, dict(null=("vel",)), EINVAL, BATCHED),
    (velocity, "nf", False, dict(frame=0), EINVAL, ONE_FRAME),
    (velocity, "nf", False, dict(null=("vel",)), ESTATE, NO_FRAME),
    (query_velocity, "nf", False, dict(frame=0), EINVAL, ONE_FRAME),
    (query_velocity, "per", False, dict(n=0), ESTATE, BEHIND_VEL),
    (query_velocity, "per", False, dict(mode=7), EINVAL, "mode must be MW_QUERY_REST or MW_QUERY_WORLD"),
    (query_velocity, "rend", False, dict(frame=0), EINVAL, "frame out of range (-1, or a frame of the latest steps call)"),
    (query_velocity, "batch", False, dict(it=-1), EINVAL, "iterations must be in [0,64]"),
    (query_velocity, "batch", False, dict(), EINVAL, BATCHED),
    # ---- the water column: handle, arguments, frame, then the state ----
    (query_column, None, False, dict(n=-1), EINVAL, "NULL handle"),
    (query_column, "rend", False, dict(it=65), EINVAL, NO_COLUMN_HANDLE),
    (query_column, "fm", False, dict(mode=7), EINVAL, "mode must be MW_QUERY_REST or MW_QUERY_WORLD"),
    (query_column, "fm", False, dict(frame=0), EINVAL, ONE_FRAME),
    (query_column, "fm", False, dict(), ESTATE, NO_COLUMN),
    (query_column, "fm", False, dict(n=0), ESTATE, NO_COLUMN),
    (query_column, "nf", False, dict(), ESTATE, NO_FRAME),
    (query_column, "per", False, dict(), ESTATE, NO_COLUMN),
    (query_column, "per", False, dict(column=True), ESTATE, BEHIND_COL),
    (query_column, "per", False, dict(column=True, null=("xyz",)), EINVAL, "NULL array"),
    # ---- raycasts ----
    (raycast, "per", False, dict(n=-1), EINVAL, "n < 0"),
    (raycast, "per", False, dict(null=("qout",)), EINVAL, "NULL array"),
    (raycast, "per", False, dict(n=0), ESTATE, "raycasts do not tile yet: the handle is periodic (mw_ocean_set_periodic(o, 0) first, or "
                                               "mw_ocean_raycast_tiled for the tiled surface)"),
    (raycast, "batch", False, dict(), EINVAL, BATCHED),
    (raycast, "nf", False, dict(n=0), ESTATE, NO_FRAME),
    (raycast_tiled, None, False, dict(reach=-1), EINVAL, "NULL handle"),
    (raycast_tiled, "rend", False, dict(reach=-1), ESTATE, NOT_TILING),
    (raycast_tiled, "batch", False, dict(reach=-1), EINVAL, BATCHED),
    (raycast_tiled, "fm", False, dict(reach=-1, n=-1), EINVAL, REACH),
    (raycast_tiled, "fm", False, dict(reach=2000, frame=0), EINVAL, REACH),
    (raycast_tiled, "fm", False, dict(frame=0, null=("rays",)), EINVAL, "NULL array"),
    (raycast_tiled, "nf", False, dict(n=0), ESTATE, NO_FRAME),
    # ---- hull forces ----
    (hull_forces, "batch", False, dict(nb=-1), EINVAL, BATCHED),
    (hull_forces, "fm", False, dict(nb=-1, nverts=2), EINVAL, "nbodies < 0"),
    (hull_forces, "fm", False, dict(nverts=2, null=("coeffs",)), EINVAL, "a hull needs nverts >= 3 and ntris >= 1"),
    (hull_forces, "fm", False, dict(null=("coeffs", "out")), EINVAL, "NULL coeffs"),
    (hull_forces, "nf", False, dict(coeffs="coeffs"), EINVAL, "coefficients must be finite and >= 0"),
    (hull_forces, "nf", False, dict(nb=0), ESTATE, NO_FRAME),
    (hull_forces, "nf", False, dict(tris="tris"), ESTATE, NO_FRAME),
    (hull_forces, "fm", False, dict(nb=0, tris="tris"), OK, None),
    (hull_forces, "fm", False, dict(it=65, tris="tris"), EINVAL, "iterations must be in [0,64]"),
    (hull_forces, "fm", False, dict(tris="tris"), EINVAL, TRIANGLE),
    (hull_forces, "fm", False, dict(draught=True, frame=0), EINVAL, ONE_FRAME),
    (hull_forces, "fm", False, dict(draught=True, nb=0), ESTATE, NO_COLUMN),
    (hull_forces, "fm", False, dict(draught=True, tris="tris"), ESTATE, NO_COLUMN),
    # ---- floating bodies: the call's own arguments, then the hull's ----
    (step_bodies, None, False, dict(sub=0), EINVAL, SUBSTEPS),
    (step_bodies, None, False, dict(), EINVAL, "NULL handle"),
    (step_bodies, "fm", False, dict(dt=-1.0, null=("mass",)), EINVAL, "dt must be finite and >= 0"),
    (step_bodies, "batch", False, dict(null=("mass",)), EINVAL, "NULL array"),
    (step_bodies, "batch", False, dict(nverts=2), EINVAL, BATCHED),
    (step_bodies, "fm", False, dict(tris="tris", mass="mass0"), EINVAL, TRIANGLE),
    (step_bodies, "fm", False, dict(mass="mass01"), EINVAL, mass_row(0)),
    (step_bodies, "fm", False, dict(mass="mass1"), EINVAL, mass_row(1)),
    (step_bodies, "nf", False, dict(nb=0), ESTATE, NO_FRAME),
    (step_bodies, "nf", False, dict(tris="tris", mass="mass0"), ESTATE, NO_FRAME),
    (step_bodies, "fm", False, dict(nb=0, tris="tris", mass="mass0"), OK, None),
    (step_bodies, "fm", False, dict(draught=True, mass="mass0"), ESTATE, NO_COLUMN),
    # ---- moorings: the call's own arguments, then stepping's ----
    (step_moored, None, False, dict(K=0), EINVAL, LINES),
    (step_moored, "fm", False, dict(K=9, sub=0), EINVAL, LINES),
    (step_moored, "fm", False, dict(null=("lines",), sub=0), EINVAL, "NULL lines"),
    (step_moored, None, False, dict(sub=65), EINVAL, SUBSTEPS),
    (step_moored, "fm", False, dict(tris="tris", lines="slot00"), EINVAL, TRIANGLE),
    (step_moored, "fm", False, dict(mass="mass0", lines="slot00"), EINVAL, mass_row(0)),
    (step_moored, "fm", False, dict(mass="mass1", lines="slot01"), EINVAL, slot(1, 0)),
    (step_moored, "fm", False, dict(mass="mass1", lines="slot10"), EINVAL, mass_row(1)),
    (step_moored, "fm", False, dict(lines="slot10"), EINVAL, slot(0, 1)),
    (step_moored, "nf", False, dict(nb=0, null=("lines",)), ESTATE, NO_FRAME),
    (step_moored, "fm", False, dict(nb=0, null=("lines",), tris="tris", mass="mass0"), OK, None),
    # ---- fleets: NULL handle, draught, then the call ----
    (fleet_forces, None, False, dict(nhulls=0), EINVAL, "NULL handle"),
    (step_fleet, None, False, dict(sub=0), EINVAL, "NULL handle"),
    (fleet_forces, "fm", False, dict(draught=True, nhulls=0), ESTATE, DRAUGHT),
    (step_fleet, "fm", False, dict(draught=True, sub=0), ESTATE, DRAUGHT),
    (fleet_forces, "batch", False, dict(nhulls=0), EINVAL, BATCHED),
    (step_fleet, "fm", False, dict(sub=0, nhulls=0), EINVAL, SUBSTEPS),
    (fleet_forces, "fm", False, dict(nhulls=0, null=("coeffs",)), EINVAL, "nhulls must be in [1, MW_FLEET_MAX_HULLS]"),
    (fleet_forces, "fm", False, dict(table="table_nverts", tb=3), EINVAL, "hull 0 needs nverts >= 3 and ntris >= 1"),
    (fleet_forces, "fm", False, dict(tb=3, null=("out",)), EINVAL, "the hulls' nbodies must add up to total_bodies"),
    (fleet_forces, "fm", False, dict(null=("out",), coeffs="coeffs"), EINVAL, "NULL array"),
    (step_fleet, "fm", False, dict(null=("mass",), frame=0), EINVAL, "NULL array"),
    (step_fleet, "fm", False, dict(tris="tris", mass="mass0"), EINVAL, "hull 0: " + TRIANGLE),
    (step_fleet, "fm", False, dict(mass="mass0", wrench="wrench0"), EINVAL, mass_row(0)),
    (step_fleet, "fm", False, dict(mass="mass1", wrench="wrench0"), EINVAL, "the wrench row of body 0 is not finite"),
    (fleet_forces, "nf", False, dict(table="table_empty", tb=0), ESTATE, NO_FRAME),
    (step_fleet, "nf", False, dict(table="table_empty", tb=0), ESTATE, NO_FRAME),
    (fleet_forces, "fm", False, dict(table="table_empty", tb=0, tris="tris"), OK, None),
    (step_fleet, "fm", False, dict(table="table_empty", tb=0, tris="tris", mass="mass0"), OK, None),
]


def _name(row):
    fn, handle, dev, kw = row[:4]
    return f"{fn.__name__}{'_device' if dev else ''}-{handle}-" + ",".join(f"{k}={v}" for k, v in kw.items())


def run_row(cx, row):
    """(status, mw_last_error()) of a row's call"""
    fn, handle, dev, kw = row[:4]
    kw = dict(kw)
    o = cx.handles[handle] if handle else None
    draught, column = kw.pop("draught", False), kw.pop("column", False)
    if draught:
        o.set_draught(True)
    if column:
        o.set_column([0.0, 1.0, 3.0])
    try:
        s = fn(Call(cx, o._h if o else None, dev, kw))
        return s, cx.L.mw_last_error().decode()
    finally:
        if draught:
            o.set_draught(False)
        if column:
            cx.mw.check(cx.L.mw_ocean_set_column(o._h, None, 0))


@pytest.fixture(scope="module")
def cx(mw):
    import contextlib
    with contextlib.ExitStack() as stack:
        c = Ctx(mw, stack)
        yield c
        for o in c.handles.values():
            o.synchronize()


def test_rows_cover_every_entry_point():
    """each of the services' entry points has a host-form and a device-form row"""
    seen = {(row[0].__name__, row[2]) for row in ROWS}
    for fn in (query_surface, query_velocity, query_column, raycast, raycast_tiled, velocity, hull_forces, step_bodies, step_moored,
               fleet_forces, step_fleet):
        assert (fn.__name__, False) in seen and (fn.__name__, True) in seen, fn.__name__
    assert len({_name(r) for r in ROWS}) == len(ROWS)


@pytest.mark.parametrize("row", ROWS, ids=_name)
def test_reported_fault(cx, row):
    fn, handle, dev, kw, status, message = row
    got, text = run_row(cx, row)
    print(_name(row), got, repr(text))
    assert got == status
    if status != OK:
        assert text == f"mw_ocean_{fn.__name__}{'_device' if dev else ''}: {message}"
    assert cx.untouched()
