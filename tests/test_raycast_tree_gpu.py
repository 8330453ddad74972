"""GPU tier of the raycasts' hierarchy: the tree k_rc_build_leaves<SqMesh>, k_rc_build_leaves<SqTiled> and k_rc_build_top build on the
device (returned by the test hook mw_debug_raycast_tree, which runs the casts' own checks and the casts' own build on a tree buffer set
to NaN) against the serial build of the g++ shims (rc_build_serial) on the library's own frame, with the leaf size the hook reports.
Every node of every level must be equal as float32 values, padding nodes and the unused slots included: there is no tolerance.  The
serial build is in turn held against a numpy reference by tests/test_raycast_tree_cpu.py.

The tables below name every depth 0 to 9 on both surfaces, a 16 x 16 leaf tile that is wholly padding, and the clamp of the leaf size
at grids above 1024; the 2048^2 grid, where the clamp engages on its own, is also cast on."""
import numpy as np
import pytest

import ray_ref as RR
import ray_tiled_ref as RT
import workloads

pytestmark = pytest.mark.gpu

CHOP = 4.0   # as in test_raycast_tiled_gpu: the frame overhangs its footprint


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return RR.build_shim(str(tmp_path_factory.mktemp("rctreeg") / "librc_shim.so"))


@pytest.fixture(scope="module")
def tshim(tmp_path_factory):
    return RT.build_shim(str(tmp_path_factory.mktemp("rcttreeg") / "librct_shim.so"))


def _fft(mw, N, chop=CHOP):
    """unit_width 1, length N: the footprint casts read its one frame, the tiled casts its tiling"""
    p = workloads.fftmesh_params(N, choppiness=chop)
    return mw.Ocean(resolution=N, unit_width=1.0, length=float(N), wind=(p.wind_x, p.wind_y), amplitude=p.amplitude, choppiness=chop,
                    gravity=p.gravity, seed=3, device=0)


def _renderer(mw, res, seed=1):
    return mw.Ocean(resolution=res, unit_width=1.0, length=27.155 * res / 8, wind=(14.45, 12.0), amplitude=0.41, choppiness=1.5, mult=1.5,
                    seed=seed, semantics=mw.MW_SEM_OCEANRENDERER, device=0)


def _frames(o, N, t=1.7):
    """the frame as the footprint (RR.Mesh) and as its tiling (RT.TMesh): the same arrays"""
    v, n, c = o.evaluate(t)
    return RR.Mesh(N, v, n, c.reshape(-1), wstride=4), RT.TMesh(N, v, n, c.reshape(-1), wstride=4)


def _device_tree(mw, o, block, tiled, frame=-1):
    try:
        mw.set_switch("MW_RC_BLOCK", block)
        return o.raycast_tree(frame=frame, tiled=tiled)
    finally:
        mw.set_switch("MW_RC_BLOCK", 0)


def _serial_tree(sh, m, B, tiled):
    return RT.shim_tree(sh, m, B) if tiled else RR.shim_tree(sh, m, B)


def _check(mw, o, m, sh, tiled, rows, frame=-1):
    """rows of (MW_RC_BLOCK, B, nb, D): the hook reports that geometry and returns the serial tree of m with that B, node for node.
    Every row is run; the failure names each row that differs."""
    bad = []
    for block, B, nb, D in rows:
        what = ("tiled" if tiled else "footprint", m.N if tiled else m.R, "MW_RC_BLOCK", block, "D", D)
        box, b, n, d = _device_tree(mw, o, block, tiled, frame)
        assert (b, n, d) == (B, nb, D), (what, b, n, d)
        assert box.shape == ((4 ** (D + 1) - 1) // 3, 8), what
        ref = _serial_tree(sh, m, b, tiled)
        assert not np.isnan(ref).any(), what
        ok, diff = RR.same_tree(box, ref)
        if not ok:
            bad.append((what, diff))
            continue
        leaves = box[(4 ** D - 1) // 3:].reshape(2 ** D, 2 ** D, 8)
        pad = np.ones((2 ** D, 2 ** D), bool)
        pad[:nb, :nb] = False
        assert np.isfinite(leaves[~pad]).all() and np.isposinf(leaves[pad][:, 0:3]).all() and np.isneginf(leaves[pad][:, 4:7]).all(), what
        assert (box[:, 3] == 0).all() and (box[:, 7] == 0).all(), what
    assert not bad, ([w for w, _ in bad], bad[0])


class _Big:
    """the 1024^2 and 2048^2 handles of the module: each evaluated once, and closed before the other opens"""

    def __init__(self, mw):
        self.mw, self.N, self.o, self.m, self.tm = mw, None, None, None, None

    def get(self, N):
        if self.N != N:
            self.close()
            self.o = _fft(self.mw, N)
            self.m, self.tm = _frames(self.o, N)
            self.N = N
        return self.o, self.m, self.tm

    def close(self):
        if self.o is not None:
            self.o.close()
        self.N = self.o = self.m = self.tm = None


@pytest.fixture(scope="module")
def big(mw):
    b = _Big(mw)
    yield b
    b.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_rows(out, hit, so, sh, what):
    bad = ~((_bits(out) == _bits(so)).all(1) & (hit == sh).all(1))
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:6], out[bad][:3], so[bad][:3], hit[bad][:3], sh[bad][:3])


def _cast(o, rays, frame=-1):
    return o.raycast(rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7], frame=frame)


def _cast_tiled(o, rays, reach):
    return o.raycast_tiled(rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7], reach=reach)


# ---- the tables: (MW_RC_BLOCK, B, nb, D) per grid size, one handle per size ---------------------------------------------------------
FOOTPRINT = {
    64: [(64, 64, 1, 0), (32, 32, 2, 1), (16, 16, 4, 2), (8, 8, 8, 3),
         (4, 4, 16, 4),       # one full 16 x 16 tile, no top launch
         (3, 3, 21, 5),       # the first top launch, partly padded tiles
         (0, 2, 32, 5), (1, 1, 63, 6)],
    128: [(3, 3, 43, 6)],     # leaves 48..63 are a wholly empty tile row and column
    256: [(0, 2, 128, 7), (1, 1, 255, 8)],
}
FOOTPRINT_1024 = [(0, 2, 512, 9),     # the top kernel's full 32 x 32 level
                  (1, 2, 512, 9)]     # the clamp: B = 1 would be 1023 leaves a side
TILED = {
    16: [(16, 16, 1, 0),      # one leaf holds the seam
         (3, 3, 6, 3),        # the last leaf is the seam cell alone
         (1, 1, 16, 4)],
    64: [(0, 2, 32, 5)],
    100: [(0, 2, 50, 6), (3, 3, 34, 6)],   # B = 3: a wholly empty tile
    256: [(1, 1, 256, 8)],
}
TILED_1024 = [(0, 2, 512, 9), (1, 2, 512, 9)]
ABOVE_THE_CAP = [(0, 4, 512, 9), (1, 4, 512, 9), (8, 8, 256, 8)]   # N = 2048, both surfaces


@pytest.mark.parametrize("R", sorted(FOOTPRINT))
def test_footprint_tree_equals_the_serial_build(mw, shim, R):
    with _fft(mw, R, 1.5) as o:
        m, _ = _frames(o, R)
        _check(mw, o, m, shim, False, FOOTPRINT[R])


def test_footprint_tree_of_the_shipped_scene(mw, shim):
    p = workloads.shipped_fftmesh_scene()
    with mw.Ocean(resolution=p.N, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                  choppiness=p.choppiness, gravity=p.gravity, device=0) as o:
        v, n, c = o.evaluate(1.7)
        _check(mw, o, RR.Mesh(12, v, n, c.reshape(-1), wstride=4), shim, False, [(0, 2, 6, 3)])


def test_oceanrenderer_trees_and_a_frame_of_a_steps_call(mw, shim):
    for res, nb, D in ((8, 4, 2), (32, 16, 4)):
        with _renderer(mw, res) as r:
            r.generate_texture(0.016)
            _check(mw, r, RR.Mesh(res, *r.displace_mesh()), shim, False, [(0, 2, nb, D)])
    dts = [0.016, 0.4, 0.033]
    with _renderer(mw, 32, seed=9) as a, _renderer(mw, 32, seed=9) as b:
        a.generate_texture_steps(dts)
        b.generate_texture(dts[0])
        m0 = RR.Mesh(32, *b.displace_mesh())
        _check(mw, a, m0, shim, False, [(0, 2, 16, 4), (3, 3, 11, 4)], frame=0)
        for dt in dts[1:]:
            b.generate_texture(dt)
        m2 = RR.Mesh(32, *b.displace_mesh())
        assert not np.array_equal(m0.vert, m2.vert)
        _check(mw, a, m2, shim, False, [(0, 2, 16, 4)], frame=-1)
        _check(mw, a, m2, shim, False, [(0, 2, 16, 4)], frame=2)


@pytest.mark.parametrize("N", sorted(TILED))
def test_tile_tree_equals_the_serial_build(mw, tshim, N):
    with _fft(mw, N) as o:
        _, tm = _frames(o, N)
        _check(mw, o, tm, tshim, True, TILED[N])


def test_1024_trees_of_both_surfaces(mw, shim, tshim, big):
    o, m, tm = big.get(1024)
    _check(mw, o, m, shim, False, FOOTPRINT_1024)
    _check(mw, o, tm, tshim, True, TILED_1024)


def test_the_tree_buffer_only_grows(mw, shim, tshim, big):
    """D = 9, then D = 0 in the same buffer (whose other nodes still hold the larger tree), then D = 9 again, on both surfaces"""
    o, m, tm = big.get(1024)
    _check(mw, o, m, shim, False, [(0, 2, 512, 9), (1024, 1024, 1, 0), (0, 2, 512, 9)])
    _check(mw, o, tm, tshim, True, [(1024, 1024, 1, 0), (0, 2, 512, 9)])


@pytest.mark.parametrize("N", [64, 100])
def test_the_casts_use_the_tree_the_hook_returns(mw, shim, tshim, N):
    """the hook changes no cast; the shim's traversal through the DEVICE's boxes gives the device's rows; the device's root gives
    the overhang (how many neighbouring tiles a ray must visit) the shim's root gives"""
    with _fft(mw, N) as o:
        m, tm = _frames(o, N)
        rays = np.concatenate(list(RR.families(m.vert, N, np.random.default_rng(N), n=100).values()))
        trays = np.concatenate(list(RT.families(tm, np.random.default_rng(N + 1), n=60).values()))
        before, tbefore = _cast(o, rays), _cast_tiled(o, trays, 2)
        box, B, nb, D = o.raycast_tree()
        tbox, tB, _, _ = o.raycast_tree(tiled=True)
        _same_rows(*_cast(o, rays), *before, what="footprint, after the hook")
        _same_rows(*_cast_tiled(o, trays, 2), *tbefore, what="tiled, after the hook")
        out, hit = np.empty((len(rays), 8), np.float32), np.empty((len(rays), 2), np.int32)
        assert shim.rc_shim_trace(N, RR._p(m.vert), RR._p(m.norm), RR._p(m.white), m.wstride, B, RR._p(box), RR._p(rays), len(rays),
                                  RR._p(out), RR._p(hit)) == 0
        _same_rows(out, hit, *before, what="the shim through the device's boxes")
        assert (before[1][:, 0] >= 0).sum() > len(rays) // 5
        lo, hi, h = RT.root(tshim, tm, tB)
        assert RT.overhang_tiles(tshim, tm, tbox[0, 0:3], tbox[0, 4:7]) == h
        assert np.array_equal(tbox[0, 0:3], lo) and np.array_equal(tbox[0, 4:7], hi)


# ---- above the level cap: N = 2048, the smallest power of two where the leaf size is clamped on its own -----------------------------
def test_2048_trees_of_both_surfaces(mw, shim, tshim, big):
    o, m, tm = big.get(2048)
    _check(mw, o, m, shim, False, ABOVE_THE_CAP)
    _check(mw, o, tm, tshim, True, ABOVE_THE_CAP)


def test_2048_footprint_casts_against_the_shim(mw, shim, big):
    o, m, _ = big.get(2048)
    rays = np.concatenate(list(RR.families(m.vert, 2048, np.random.default_rng(2048), n=300).values()))
    out, hit = _cast(o, rays)
    so, sh = RR.cast(shim, m, rays, B=4)
    valid = ~np.isnan(so[:, 0])
    frac = float((sh[valid, 0] >= 0).mean())
    print("2048 footprint: rays", len(rays), "valid", int(valid.sum()), "hit fraction of the shim's rows", frac)
    assert frac > 0.2
    _same_rows(out, hit, so, sh, "2048 traversal")
    sub = np.random.default_rng(12).choice(len(rays), 16, replace=False)
    bo, bh = RR.cast(shim, m, rays[sub], brute=True)
    _same_rows(out[sub], hit[sub], bo, bh, "2048 brute force")
    try:
        for block in (1, 8):
            mw.set_switch("MW_RC_BLOCK", block)
            _same_rows(*_cast(o, rays), out, hit, ("2048, MW_RC_BLOCK", block))
    finally:
        mw.set_switch("MW_RC_BLOCK", 0)


def test_2048_tiled_casts_against_the_shim(mw, tshim, big):
    o, _, tm = big.get(2048)
    rays = np.concatenate(list(RT.families(tm, np.random.default_rng(2049), n=60).values()))
    for reach in (0, 2):
        out, hit = _cast_tiled(o, rays, reach)
        so, sh = RT.cast(tshim, tm, rays, reach, B=4)
        valid = ~np.isnan(so[:, 0])
        frac = float((sh[valid, 0] >= 0).mean())
        print("2048 tiled: reach", reach, "rays", len(rays), "valid", int(valid.sum()), "hit fraction of the shim's rows", frac)
        assert frac > 0.2
        _same_rows(out, hit, so, sh, ("2048 tiled", reach))
        try:
            for block in (1, 8):
                mw.set_switch("MW_RC_BLOCK", block)
                _same_rows(*_cast_tiled(o, rays, reach), out, hit, ("2048 tiled, MW_RC_BLOCK", block, reach))
        finally:
            mw.set_switch("MW_RC_BLOCK", 0)


# ---- the hook's statuses are the casts' -------------------------------------------------------------------------------------------
def test_statuses_of_the_hook_on_real_handles(mw):
    L = mw.lib()
    rays = RR.pack(np.tile([0.0, 50.0, 0.0], (2, 1)), [0.0, -1.0, 0.0])
    out, hit = np.zeros((2, 8), np.float32), np.zeros((2, 4), np.int32)
    geom = np.zeros(3, np.int32)

    def hook(o, tiled, frame=-1, box=None, cap=0):
        geom.fill(-7)
        return L.mw_debug_raycast_tree(o.handle, frame, tiled, None if box is None else box.ctypes.data, cap, geom.ctypes.data)

    def cast(o, tiled, frame=-1):
        if tiled:
            return L.mw_ocean_raycast_tiled(o.handle, frame, rays.ctypes.data, 2, 1, out.ctypes.data, hit.ctypes.data)
        return L.mw_ocean_raycast(o.handle, frame, rays.ctypes.data, 2, out.ctypes.data, hit.ctypes.data)

    def both(o, tiled, frame=-1):
        s = hook(o, tiled, frame)
        assert s == cast(o, tiled, frame), (tiled, frame, s)
        if s != mw.MW_OK:
            assert (geom == -7).all()
        return s

    with _fft(mw, 64) as o:
        assert both(o, 0) == mw.MW_ESTATE and both(o, 1) == mw.MW_ESTATE          # no frame yet
        o.evaluate(1.0)
        assert both(o, 0) == mw.MW_OK and list(geom) == [2, 32, 5]
        assert both(o, 1) == mw.MW_OK and list(geom) == [2, 32, 5]
        assert both(o, 0, frame=0) == mw.MW_EINVAL and both(o, 1, frame=0) == mw.MW_EINVAL
        nodes = (4 ** 6 - 1) // 3
        box = np.full((nodes, 8), 5.0, np.float32)
        assert hook(o, 0, box=box, cap=nodes - 1) == mw.MW_EINVAL and (box == 5.0).all() and list(geom) == [2, 32, 5]
        assert hook(o, 1, box=box, cap=0) == mw.MW_EINVAL and (box == 5.0).all()
        assert hook(o, 0, box=box, cap=nodes) == mw.MW_OK and np.isfinite(box).all()
        assert L.mw_debug_raycast_tree(o.handle, -1, 0, box.ctypes.data, nodes, None) == mw.MW_EINVAL
        o.set_periodic(True)
        assert both(o, 0) == mw.MW_ESTATE and b"do not tile" in L.mw_last_error()  # a periodic handle has no one footprint
        assert both(o, 1) == mw.MW_OK
        o.set_periodic(False)
        assert both(o, 0) == mw.MW_OK
    p = workloads.shipped_fftmesh_scene()
    with mw.Ocean(resolution=p.N, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                  choppiness=p.choppiness, gravity=p.gravity, device=0) as o:
        o.evaluate(1.0)
        assert both(o, 1) == mw.MW_ENOTCOMMENSURATE                                # N = 12, length 12.39
        assert both(o, 0) == mw.MW_OK and list(geom) == [2, 6, 3]
    kw = dict(resolution=8, length=27.155, wind=(14.45, 12.0), amplitude=0.41, choppiness=0.46, mult=1.5, semantics=mw.MW_SEM_OCEANRENDERER,
              device=0)
    with mw.Ocean(**kw) as r:
        assert both(r, 0) == mw.MW_ESTATE                                          # no GenerateTexture() yet
        r.generate_texture(0.1)
        assert both(r, 1) == mw.MW_ESTATE                                          # an OceanRenderer mesh does not tile
        assert both(r, 0) == mw.MW_OK and list(geom) == [2, 4, 2]
        assert both(r, 0, frame=0) == mw.MW_EINVAL                                 # no steps call yet
    with mw.Ocean(ntiles=2, **kw) as t:
        t.generate_texture(0.1)
        assert both(t, 0) == mw.MW_EINVAL and both(t, 1) == mw.MW_EINVAL           # batched handles have no single surface
