"""CPU tier of the raycasts' hierarchy (csrc/raycast.h): the serial build the GPU tier holds the device against (rc_build_serial, through
tests/raycast_shim.cpp and tests/raycast_tiled_shim.cpp) against ray_ref.tree_ref, a numpy float32 restatement of the tree written from
the header's comment: every node of every level equal as float32 values, padding leaves and the unused slots included.  No tolerance:
min and max are exact, and the padding is four float32 operations in a stated order."""
import numpy as np
import pytest

import ray_ref as RR
import ray_tiled_ref as RT


@pytest.fixture(scope="module")
def shim(tmp_path_factory):
    return RR.build_shim(str(tmp_path_factory.mktemp("rctree") / "librc_shim.so"))


@pytest.fixture(scope="module")
def tshim(tmp_path_factory):
    return RT.build_shim(str(tmp_path_factory.mktemp("rcttree") / "librct_shim.so"))


def _assert_tree(got, ref, what):
    assert not np.isnan(ref).any(), what
    ok, diff = RR.same_tree(got, ref)
    assert ok, (what, diff)
    assert (got[:, 3] == 0).all() and (got[:, 7] == 0).all(), what


# (R, B) -> (nb, D): one cell; one leaf cut at the last line; the shipped scene's size; partly padded levels; a leaf of 64 cells
FOOTPRINT = [(2, 2, 1, 0), (3, 2, 1, 0), (12, 2, 6, 3), (64, 3, 21, 5), (130, 5, 26, 5), (130, 64, 3, 2)]
# (N, B) -> (nb, D): one leaf holds both seams; the last leaf is the seam cell alone; padding leaves
TILED = [(16, 16, 1, 0), (16, 3, 6, 3), (100, 3, 34, 6)]


@pytest.mark.parametrize("kind", ["rough", "choppy", "flat", "far"])
@pytest.mark.parametrize("R,B,nb,D", FOOTPRINT)
def test_the_serial_footprint_tree_equals_the_numpy_reference(shim, R, B, nb, D, kind):
    m = RR.synthetic(R, kind, seed=R + B)
    ref, rnb, rD = RR.tree_ref(m.vert.reshape(R, R, 3), B)
    assert (rnb, rD) == (nb, D) and shim.rc_shim_nodes(R, B) == len(ref)
    got = RR.shim_tree(shim, m, B)
    _assert_tree(got, ref, (R, B, kind))
    leaves = got[(4 ** D - 1) // 3:].reshape(2 ** D, 2 ** D, 8)
    assert np.isfinite(leaves[:nb, :nb]).all()
    if kind == "flat":       # y = 0 exactly: nothing to pad by
        assert (leaves[:nb, :nb, 1] == 0).all() and (leaves[:nb, :nb, 5] == 0).all() and got[0, 1] == 0 and got[0, 5] == 0
    if kind == "far":        # the magnitude term is the padding: far above PAD times the extent of a leaf
        ext = leaves[:nb, :nb, 4] - leaves[:nb, :nb, 0]
        assert (leaves[:nb, :nb, 0] > 9.0e3).all() and (ext > 2 * RR.PAD * 9.0e3).all()


@pytest.mark.parametrize("kind", ["rough", "folded", "big", "level", "far"])
@pytest.mark.parametrize("N,B,nb,D", TILED)
def test_the_serial_tile_tree_equals_the_numpy_reference(tshim, N, B, nb, D, kind):
    m = RT.synthetic(N, kind, seed=N + B)
    ref, rnb, rD = RR.tree_ref(RT.tile_grid(m), B)
    assert (rnb, rD) == (nb, D) and tshim.rct_shim_nodes(N, B) == len(ref)
    got = RT.shim_tree(tshim, m, B)
    _assert_tree(got, ref, (N, B, kind))
    if kind == "level":
        assert got[0, 1] == 0 and got[0, 5] == 0
    lo, hi, h = RT.root(tshim, m, B)
    assert np.array_equal(lo, ref[0, 0:3]) and np.array_equal(hi, ref[0, 4:7]) and RT.overhang_tiles(tshim, m, lo, hi) == h


def test_the_reference_holds_what_the_comment_says_on_a_mesh_small_enough_to_write_out():
    """tree_ref against boxes worked out by hand: 3 x 3 grid lines, B = 1 (four leaves of one cell, D = 1), coordinates whose float32
    padding is exact (powers of two)"""
    g = np.zeros((3, 3, 3), np.float32)
    for i in range(3):
        for j in range(3):
            g[i, j] = (4.0 * i, 0.0, 4.0 * j)
    g[1, 1, 1] = 8.0
    box, nb, D = RR.tree_ref(g, 1)
    assert (nb, D, len(box)) == (2, 1, 5)
    p = 2.0 ** -14
    # leaf (0, 0): x and z in [0, 4] (extent 4 + magnitude 4), y in [0, 8] (8 + 8)
    assert np.array_equal(box[1], np.array([-8 * p, -16 * p, -8 * p, 0, 4 + 8 * p, 8 + 16 * p, 4 + 8 * p, 0], np.float32))
    # leaf (1, 0) = node 3: x in [4, 8] (4 + 8), z in [0, 4]
    assert np.array_equal(box[3], np.array([4 - 12 * p, -16 * p, -8 * p, 0, 8 + 12 * p, 8 + 16 * p, 4 + 8 * p, 0], np.float32))
    assert np.array_equal(box[0], np.array([-8 * p, -16 * p, -8 * p, 0, 8 + 12 * p, 8 + 16 * p, 8 + 12 * p, 0], np.float32))
    box, nb, D = RR.tree_ref(g, 2)                      # one leaf: x in [0, 8] (8 + 8)
    assert (nb, D) == (1, 0) and np.array_equal(box[0], np.array([-16 * p, -16 * p, -16 * p, 0, 8 + 16 * p, 8 + 16 * p, 8 + 16 * p, 0],
                                                                 np.float32))
    box, nb, D = RR.tree_ref(np.concatenate([np.concatenate([g, g[:, :1]], 1), np.concatenate([g, g[:, :1]], 1)[:1]], 0), 1)
    assert (nb, D, len(box)) == (3, 2, 21) and np.isposinf(box[5 + 3, 0]) and np.isneginf(box[5 + 15, 6])   # leaves (0, 3), (3, 3)


def test_hook_is_exported_declared_and_refuses_a_null_handle(mw):
    from mistral_water import _native
    L = mw.lib()
    assert "mw_debug_raycast_tree" in _native.HOOK_SYMBOLS and "mw_debug_raycast_tree" not in _native.ABI_SYMBOLS
    geom = np.full(3, 7, np.int32)
    for tiled in (0, 1):
        assert L.mw_debug_raycast_tree(None, -1, tiled, None, 0, geom.ctypes.data) == mw.MW_EINVAL
        assert b"NULL handle" in L.mw_last_error() and (geom == 7).all()
    assert L.mw_debug_raycast_tree(None, -1, 0, None, 0, None) == mw.MW_EINVAL
