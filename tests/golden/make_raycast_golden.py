"""Writes tests/golden/raycast_rows.npz: the rows and hierarchies of both raycasts (csrc/raycast.h, csrc/raycast_tiled.h) as the g++
shims of the checkout this file sits in compute them.  tests/test_raycast_golden_cpu.py holds every later state of the headers to these
bits, so run it on the commit whose bits are to be kept:

    python tests/golden/make_raycast_golden.py [--out FILE]

Per case the file holds the mesh arrays, the rays (the tests' families plus four invalid rays), out / hit of the hierarchy cast at leaf
size B = 2 and the whole box array; for the tiling also rct_shim_root's root box, x0 and h."""
import argparse
import ctypes as C
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import ray_ref as RR  # noqa: E402
import ray_tiled_ref as RT  # noqa: E402
import surface_ref as S  # noqa: E402

B = 2
FOOTPRINT = [(17, 0.6), (17, 1.8)]                                           # synth_mesh(R, 1.0, fold, seed=17)
TILED = [(16, "folded", 1, 1.0, 1), (8, "big", 2, 1.0, 2), (6, "rough", 3, 0.75, 0)]  # synthetic(N, kind, seed, uw), reach


def invalid_rays():
    """a NaN origin, an infinite direction component, d = 0, tmin > tmax"""
    return np.concatenate([RR.pack([np.nan, 1.0, 0.0], [0.0, -1.0, 0.0]), RR.pack([0.0, 1.0, 0.0], [0.0, -np.inf, 0.3]),
                           RR.pack([0.0, 1.0, 0.0], [0.0, 0.0, 0.0]), RR.pack([0.0, 1.0, 0.0], [0.0, -1.0, 0.0], 2.0, 1.0)])


def footprint_inputs(k):
    R, fold = FOOTPRINT[k]
    vert, norm, white = S.synth_mesh(R, 1.0, fold, seed=17)
    m = RR.Mesh(R, vert, norm, white)
    rays = np.concatenate(list(RR.families(m.vert, R, np.random.default_rng(18), n=40).values()) + [invalid_rays()])
    return m, np.ascontiguousarray(rays, np.float32)


def tiled_inputs(k):
    N, kind, seed, uw, reach = TILED[k]
    m = RT.synthetic(N, kind, seed, uw)
    rays = np.concatenate(list(RT.families(m, np.random.default_rng(100 + k), n=40).values()) + [invalid_rays()])
    return m, np.ascontiguousarray(rays, np.float32), reach


def footprint_results(L, m, rays):
    """what the footprint's shim makes of (mesh, rays): out, hit, box"""
    box = np.empty((L.rc_shim_nodes(m.R, B), 8), np.float32)
    assert L.rc_shim_build(m.R, RR._p(m.vert), B, RR._p(box)) == 0
    out, hit = RR.cast(L, m, rays, B=B)
    return {"out": out, "hit": hit, "box": box}


def tiled_results(L, m, rays, reach):
    """what the tiling's shim makes of (mesh, rays, reach): out, hit, box, root [6], x0, h"""
    box = np.empty((L.rct_shim_nodes(m.N, B), 8), np.float32)
    assert L.rct_shim_build(m.N, m.uw, m.P, RR._p(m.vert), B, RR._p(box)) == 0
    r6, x0, h = np.empty(6, np.float32), C.c_float(0), C.c_int32(0)
    assert L.rct_shim_root(m.N, m.uw, m.P, RR._p(m.vert), B, RR._p(r6), C.byref(x0), C.byref(h)) == 0
    out, hit = RT.cast(L, m, rays, reach, B=B)
    return {"out": out, "hit": hit, "box": box, "root": r6, "x0": np.float32(x0.value), "h": np.int32(h.value)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(HERE, "raycast_rows.npz"))
    args = ap.parse_args()
    tmp = tempfile.mkdtemp()
    L1, LT = RR.build_shim(os.path.join(tmp, "librc_shim.so")), RT.build_shim(os.path.join(tmp, "librct_shim.so"))
    z = {}
    for k in range(len(FOOTPRINT)):
        m, rays = footprint_inputs(k)
        res = footprint_results(L1, m, rays)
        z.update({"fp%d_%s" % (k, n): a for n, a in
                  dict(res, R=np.int32(m.R), vert=m.vert, norm=m.norm, white=m.white, rays=rays).items()})
        hit = res["hit"][:-4]
        print("footprint %d: %d hits, %d misses, %d from below" % (k, (hit[:, 0] >= 0).sum(), (hit[:, 0] < 0).sum(), (hit[:, 1] < 0).sum()))
    for k in range(len(TILED)):
        m, rays, reach = tiled_inputs(k)
        res = tiled_results(LT, m, rays, reach)
        z.update({"tl%d_%s" % (k, n): a for n, a in
                  dict(res, N=np.int32(m.N), uw=np.float32(m.uw), reach=np.int32(reach), vert=m.vert, norm=m.norm, white=m.white,
                       rays=rays).items()})
        hit, h = res["hit"][:-4], res["hit"][:-4, 0] >= 0
        K0 = np.floor((rays[:-4][:, [0, 2]].astype(np.float64) - m.x0) / m.P)
        cell = hit[:, 0] >> 1
        print("tiled %d: %d hits, %d in another tile, %d seam, %d out of reach, h = %d"
              % (k, h.sum(), (h & ((hit[:, 2] != K0[:, 0]) | (hit[:, 3] != K0[:, 1]))).sum(),
                 (h & ((cell // m.N == m.N - 1) | (cell % m.N == m.N - 1))).sum(), (hit[:, 0] == RT.OUT_OF_REACH).sum(), res["h"]))
    np.savez_compressed(args.out, **z)
    print("%s: %d bytes" % (args.out, os.path.getsize(args.out)))


if __name__ == "__main__":
    main()
