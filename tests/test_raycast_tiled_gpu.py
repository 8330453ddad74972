"""GPU tier of the tiled raycasts (mw_ocean_raycast_tiled / _device, include/mistral_water.h) through the C ABI.

The reference is the g++ build of the same MW_HD functions (tests/raycast_tiled_shim.cpp) run on the library's own vertex arrays: every
row must match it bit for bit, in the host and device forms, with and without a hit array, for windows of reach 0, 2 and 16, on FFTMesh
grids whose tree has 3 levels (N = 16), takes the top-level build kernel (N = 64) and has padding leaves (the chirp-z grid N = 100).
Also: leaf sizes that do not divide N, independence of the periodic switch, no state change, every status."""
import numpy as np
import pytest

import ray_ref as RR
import ray_tiled_ref as RT
import workloads

pytestmark = pytest.mark.gpu

CHOP = 4.0      # choppy enough that the 64^2 and 100^2 frames overhang their footprint by more than a cell (asserted below)
REACHES = (0, 2, 16)
_overhang = {}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return RT.build_shim(str(tmp_path_factory.mktemp("rctg") / "librct_shim.so"))


def _ocean(mw, N, chop=CHOP):
    p = workloads.fftmesh_params(N, choppiness=chop)
    return mw.Ocean(resolution=N, unit_width=1.0, length=float(N), wind=(p.wind_x, p.wind_y), amplitude=p.amplitude, choppiness=chop,
                    gravity=p.gravity, seed=3, device=0)


def _frame(o, N, t=1.7):
    v, n, c = o.evaluate(t)
    return RT.TMesh(N, v, n, c.reshape(-1), wstride=4)


def _cast(o, rays, reach):
    return o.raycast_tiled(rays[:, 0:3], rays[:, 4:7], rays[:, 3], rays[:, 7], reach=reach)


def _same(out, hit, so, sh, what=""):
    bad = ~((RT.bits(out) == RT.bits(so)).all(1) & (hit == sh).all(1))
    assert not bad.any(), (what, int(bad.sum()), np.flatnonzero(bad)[:6], out[bad][:3], so[bad][:3], hit[bad][:3], sh[bad][:3])


def _device(o, rays, reach, with_hit=True):
    import torch
    d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
    d_out = torch.full((len(rays), 8), 7.0, device="cuda")
    d_hit = torch.full((len(rays), 4), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    o.raycast_tiled_device(d_rays.data_ptr(), len(rays), d_out.data_ptr(), d_hit.data_ptr() if with_hit else 0, reach=reach)
    o.synchronize()
    return d_out.cpu().numpy(), d_hit.cpu().numpy()


def _check_mesh(mw, shim, N, blocks=(0,)):
    """the families on one frame: host and device forms against the shim for every reach (and leaf size); the conditions that keep the
    comparison from passing on rays that see nothing"""
    with _ocean(mw, N) as o:
        m = _frame(o, N)
        lo, hi, h = RT.root(shim, m)
        _overhang[N] = float(max(m.x0 - lo[0], hi[0] - (m.x0 + m.P), m.x0 - lo[2], hi[2] - (m.x0 + m.P)))
        fam = RT.families(m, np.random.default_rng(N), n=150)
        names = np.concatenate([[k] * len(v) for k, v in fam.items()])
        rays = np.concatenate(list(fam.values()))
        assert len(rays) <= 3000
        hits = valid = other = seam = oor_n = 0
        fam_hits = dict.fromkeys(fam, 0)
        try:
            for B in blocks:
                mw.set_switch("MW_RC_BLOCK", B)
                for reach in REACHES:
                    so, sh = RT.cast(shim, m, rays, reach, B=B or 2)
                    out, hit = _cast(o, rays, reach)
                    _same(out, hit, so, sh, (N, B, reach, "host"))
                    if B == 0:
                        dout, dhit = _device(o, rays, reach)
                        _same(dout, dhit, so, sh, (N, reach, "device"))
                        dout, dhit = _device(o, rays, reach, with_hit=False)
                        assert np.array_equal(RT.bits(dout), RT.bits(so)) and (dhit == 7).all(), (N, reach, "device, no hit array")
                        out2 = np.empty_like(out)
                        assert mw.lib().mw_ocean_raycast_tiled(o.handle, -1, rays.ctypes.data, len(rays), reach, out2.ctypes.data, None) == mw.MW_OK
                        assert np.array_equal(RT.bits(out2), RT.bits(so)), (N, reach, "host, no hit array")
                    hh = sh[:, 0] >= 0
                    for name in fam:
                        fam_hits[name] += int(hh[names == name].sum())
                    hits += int(hh.sum())
                    valid += int((~np.isnan(so[:, 0])).sum())
                    K0 = np.floor((rays[:, [0, 2]].astype(np.float64) - m.x0) / m.P)
                    other += int((hh & ((sh[:, 2] != K0[:, 0]) | (sh[:, 3] != K0[:, 1]))).sum())
                    cell = sh[:, 0] >> 1
                    seam += int((hh & ((cell // N == N - 1) | (cell % N == N - 1))).sum())
                    oor = sh[:, 0] == RT.OUT_OF_REACH
                    oor_n += int(oor.sum())
                    if N == 16 and oor.any():                    # nothing in the window: the brute force over all its tiles agrees
                        bo, bh = RT.cast(shim, m, rays[oor][:64], reach, brute=True)
                        assert (bh[:, 0] == -1).all()
        finally:
            mw.set_switch("MW_RC_BLOCK", 0)
        assert all(fam_hits.values()), fam_hits
        assert hits >= 0.25 * valid and other > 0 and seam > 0 and oor_n > 0, (N, hits, valid, other, seam, oor_n)


def test_n16_three_levels_and_leaf_sizes_that_do_not_divide_n(mw, shim):
    """N = 16, B = 2: D = 3, no top-level build kernel; MW_RC_BLOCK 1 (D = 4) and 3 (the last leaf holds the seam and is not full)"""
    _check_mesh(mw, shim, 16, blocks=(0, 1, 3))


def test_n64_takes_the_top_level_build_kernel(mw, shim):
    _check_mesh(mw, shim, 64)


def test_n100_chirp_z_grid_with_padding_leaves(mw, shim):
    _check_mesh(mw, shim, 100)


def test_a_frame_overhangs_its_footprint_by_more_than_a_cell(mw, shim):
    for N in (64, 100):
        if N not in _overhang:
            with _ocean(mw, N) as o:
                m = _frame(o, N)
                lo, hi, _ = RT.root(shim, m)
                _overhang[N] = float(max(m.x0 - lo[0], hi[0] - (m.x0 + m.P), m.x0 - lo[2], hi[2] - (m.x0 + m.P)))
    assert max(_overhang.values()) > 1.0, _overhang


def test_the_switch_is_neither_read_nor_changed(mw, shim):
    N = 64
    with _ocean(mw, N) as o:
        m = _frame(o, N)
        o.set_timer(3.5)
        rays = np.concatenate(list(RT.families(m, np.random.default_rng(1), n=100).values()))
        inside = RR.pack(np.random.default_rng(2).uniform([-20, 3, -20], [20, 6, 20], (500, 3)), [0.1, -1.0, 0.2])
        before = o.raycast(inside[:, 0:3], inside[:, 4:7])
        off = _cast(o, rays, 2)
        assert not o.periodic and o.timer == 3.5
        o.set_periodic(True)
        on = _cast(o, rays, 2)
        assert o.periodic and o.timer == 3.5
        _same(*on, *off, what="switch on")
        L = mw.lib()
        out, hit = np.full((len(inside), 8), 5.0, np.float32), np.full((len(inside), 2), 5, np.int32)
        assert L.mw_ocean_raycast(o.handle, -1, inside.ctypes.data, len(inside), out.ctypes.data, hit.ctypes.data) == mw.MW_ESTATE
        assert b"do not tile" in L.mw_last_error() and (out == 5.0).all() and (hit == 5).all()
        o.set_periodic(False)
        _same(*_cast(o, rays, 2), *off, what="switch off again")
        after = o.raycast(inside[:, 0:3], inside[:, 4:7])
        assert np.array_equal(RT.bits(after[0]), RT.bits(before[0])) and np.array_equal(after[1], before[1])
        assert not o.periodic and o.timer == 3.5
        for x, y in zip(o.evaluate(1.7), (m.vert, m.norm)):
            assert np.array_equal(RT.bits(x.reshape(-1)), RT.bits(y.reshape(-1)))


def test_statuses(mw):
    import torch
    L = mw.lib()
    rays = RR.pack(np.tile([0.0, 50.0, 0.0], (4, 1)), [0.0, -1.0, 0.0])
    out = np.full((4, 8), 5.0, np.float32)
    hit = np.full((4, 4), 5, np.int32)

    def st(o, frame=-1, n=4, reach=1, a=rays, b=out, h=hit):
        out.fill(5.0)
        hit.fill(5)
        s = L.mw_ocean_raycast_tiled(o.handle, frame, None if a is None else a.ctypes.data, n, reach, None if b is None else b.ctypes.data,
                                     None if h is None else h.ctypes.data)
        if s != mw.MW_OK:
            assert (out == 5.0).all() and (hit == 5).all()       # caller buffers untouched on failure
        return s
    with _ocean(mw, 16, 1.0) as o:
        assert st(o) == mw.MW_ESTATE                             # no frame yet
        o.evaluate(1.0)
        assert st(o, frame=0) == mw.MW_EINVAL
        assert st(o, reach=-1) == mw.MW_EINVAL and st(o, reach=mw.MW_RC_MAX_REACH + 1) == mw.MW_EINVAL
        assert st(o, a=None) == mw.MW_EINVAL and st(o, b=None) == mw.MW_EINVAL
        assert st(o, n=-1) == mw.MW_EINVAL and st(o, n=2 ** 32) == mw.MW_EINVAL
        assert st(o, n=0, a=None, b=None, h=None) == mw.MW_OK and (out == 5.0).all()
        d = torch.zeros(64, device="cuda")
        p0 = d.data_ptr()
        dev = L.mw_ocean_raycast_tiled_device
        assert dev(o.handle, -1, p0 + 4, 1, 1, p0 + 64, p0 + 128) == mw.MW_EINVAL     # d_rays not 16-byte aligned
        assert dev(o.handle, -1, p0, 1, 1, p0 + 72, p0 + 128) == mw.MW_EINVAL         # d_out
        assert dev(o.handle, -1, p0, 1, 1, p0 + 64, p0 + 136) == mw.MW_EINVAL         # d_hit
        assert dev(o.handle, -1, p0, 1, 1, p0 + 64, p0 + 128) == mw.MW_OK
        o.synchronize()
        assert st(o, reach=0, h=None) == mw.MW_OK and np.isfinite(out).all() and (hit == 5).all()
        assert st(o, reach=mw.MW_RC_MAX_REACH) == mw.MW_OK
        assert (hit[:, 0] >= 0).all() and (hit[:, 2:] == 0).all() and np.isfinite(out).all()   # straight down from above: the water
    with _ocean_params(mw, workloads.shipped_fftmesh_scene()) as o:
        o.evaluate(1.0)
        assert st(o) == mw.MW_ENOTCOMMENSURATE                   # N = 12, length 12.39
    with mw.Ocean(resolution=9, unit_width=1.0, length=9.0, device=0) as o:
        o.evaluate(1.0)
        assert st(o) == mw.MW_ENOTCOMMENSURATE                   # an odd N is anti-periodic
    kw = dict(resolution=8, length=27.155, wind=(14.45, 12.0), amplitude=0.41, choppiness=0.46, mult=1.5, semantics=mw.MW_SEM_OCEANRENDERER,
              device=0)
    with mw.Ocean(**kw) as r:
        r.generate_texture(0.1)
        assert st(r) == mw.MW_ESTATE
    with mw.Ocean(ntiles=2, **kw) as t:
        t.generate_texture(0.1)
        assert st(t) == mw.MW_EINVAL                             # batched handles have no single surface


def _ocean_params(mw, p):
    return mw.Ocean(resolution=p.N, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                    choppiness=p.choppiness, gravity=p.gravity, device=0)
