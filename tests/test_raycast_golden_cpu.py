"""Both raycasts held to recorded bits (tests/golden/raycast_rows.npz, written by tests/golden/make_raycast_golden.py from the commit
before csrc/raycast.h and csrc/raycast_tiled.h came to share their leaf box, cell test, sibling step and hit row).

The other raycast tests compare the device with the shim and the shim's walk with the shim's brute force: all of them build from the
same headers, so a change of the arithmetic made consistently passes them.  Here the rows, the hit records and the whole hierarchy of
the g++ shims built from the working tree must equal the recorded ones bit for bit (uint32 views: the NaN rows compare too), the brute
force must give the same rows, and the fixture itself must see enough -- hits, misses, other tiles, seams, out-of-reach rows, invalid
rays, an overhang of two periods -- for that to mean something."""
import importlib.util
import os

import numpy as np
import pytest

import ray_ref as RR
import ray_tiled_ref as RT

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_raycast_golden", os.path.join(GOLDEN, "make_raycast_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(GOLDEN, "raycast_rows.npz")) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return RR.build_shim(str(tmp_path_factory.mktemp("rcg") / "librc_shim.so"))


@pytest.fixture(scope="module")
def tiled_shim(tmp_path_factory):
    return RT.build_shim(str(tmp_path_factory.mktemp("rctg") / "librct_shim.so"))


def _bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype.itemsize == 4, a.dtype
    return a.view(np.uint32)


def _same(got, want, what):
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    diff = _bits(got) != _bits(want)
    assert not diff.any(), (what, int(diff.sum()), np.argwhere(diff)[:4].tolist())


def _case(golden, prefix):
    return {k[len(prefix):]: v for k, v in golden.items() if k.startswith(prefix)}


def _fixture_sees_enough(c):
    """at least a quarter of the valid rays hit, at least one misses, exactly four rows are invalid (all NaN)"""
    out, hit = c["out"], c["hit"]
    invalid = np.isnan(out[:, 0])
    assert invalid.sum() == 4 and invalid[-4:].all() and np.isnan(out[invalid]).all() and (hit[invalid, 0] == -1).all()
    hits, misses = hit[:, 0] >= 0, np.isposinf(out[:, 0])
    assert (hits | misses | invalid).all() and np.isfinite(out[hits]).all()
    assert hits.sum() >= 0.25 * (~invalid).sum() and misses.sum() >= 1, (int(hits.sum()), int(misses.sum()))


@pytest.mark.parametrize("k", range(len(G.FOOTPRINT)))
def test_footprint_rows_and_hierarchy_keep_their_bits(golden, shim, k):
    c = _case(golden, "fp%d_" % k)
    _fixture_sees_enough(c)
    assert (c["hit"][:, 1] < 0).sum() > 0, "hits from below"
    m = RR.Mesh(int(c["R"]), c["vert"], c["norm"], c["white"])
    got = G.footprint_results(shim, m, c["rays"])
    assert set(got) == {"out", "hit", "box"}
    for name, a in got.items():
        _same(a, c[name], name)
    bo, bh = RR.cast(shim, m, c["rays"], brute=True)
    _same(bo, c["out"], "brute out")
    _same(bh, c["hit"], "brute hit")


@pytest.mark.parametrize("k", range(len(G.TILED)))
def test_tiled_rows_and_hierarchy_keep_their_bits(golden, tiled_shim, k):
    c = _case(golden, "tl%d_" % k)
    _fixture_sees_enough(c)
    N, reach, hit, rays = int(c["N"]), int(c["reach"]), c["hit"], c["rays"]
    m = RT.TMesh(N, c["vert"], c["norm"], c["white"], uw=float(c["uw"]))
    if k < 2:
        h = hit[:, 0] >= 0
        K0 = np.floor((rays[:, [0, 2]].astype(np.float64) - m.x0) / m.P)
        cell = hit[:, 0] >> 1
        assert (h & ((hit[:, 2] != K0[:, 0]) | (hit[:, 3] != K0[:, 1]))).sum() > 0, "hits in a tile other than the origin's"
        assert (h & ((cell // N == N - 1) | (cell % N == N - 1))).sum() > 0, "seam-cell hits"
        assert (hit[:, 0] == RT.OUT_OF_REACH).sum() > 0, "out-of-reach rows"
    if k == 1:
        assert int(c["h"]) == 2
    got = G.tiled_results(tiled_shim, m, rays, reach)
    assert set(got) == {"out", "hit", "box", "root", "x0", "h"}
    for name, a in got.items():
        _same(np.asarray(a), c[name], name)
    bo, bh = RT.cast(tiled_shim, m, rays, reach, brute=True)
    _same(bo, c["out"], "brute out")
    want = hit.copy()
    want[want[:, 0] == RT.OUT_OF_REACH, 0] = -1  # the brute force reports no hit as -1 always
    _same(bh, want, "brute hit")
