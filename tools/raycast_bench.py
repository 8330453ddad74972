"""Raycast timing (mw_ocean_raycast_device) on the surfaces tools/query_bench.py uses (the 1024^2 FFTMesh and OceanRenderer resolution
128): one JSON line.  HIP events around back-to-back calls on the handle's stream (torch's current stream), median and min of --reps.

  build+1    one call with a single ray: the hierarchy's launches plus one lane of k_raycast (no call builds without casting)
  camera     10^6 rays of a 1000 x 1000 perspective camera 20 m above the sea (90 degrees across, pitched 20 degrees down), pixel order
  random     10^6 rays from random points over the footprint (y in [-5, 30]) in random directions
  vertical   10^6 down-rays at random (x, z), against query_surface_device in world mode at the same points
  blocks     the same calls for every leaf size of --blocks (switch MW_RC_BLOCK; the first hit does not depend on it)
  cpu        the g++ build of the same traversal (tests/raycast_shim.cpp) on one host core: --cpu-rays rays per family, per 10^6

Usage: python tools/raycast_bench.py [--reps 20] [--blocks 2,4,8,16] [--cpu-rays 20000]"""
import argparse
import json
import os
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mistral-water_amd"), os.path.join(REPO, "tests")]
import torch  # noqa: E402  (initialises its HIP runtime before the library)

import numpy as np  # noqa: E402
import mistral_water as mw  # noqa: E402
from mistral_water import _native as nat  # noqa: E402
import ray_ref as RR  # noqa: E402
import workloads  # noqa: E402

N_RAYS = 1000 * 1000


def timed(stream, reps, fn):
    for _ in range(3):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    per = []
    for _ in range(reps):
        ev[0].record(stream)
        fn()
        ev[1].record(stream)
        ev[1].synchronize()
        per.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return round(float(np.median(per)), 1), round(float(np.min(per)), 1)


def camera_rays(side, eye, pitch_deg=20.0, fov_deg=90.0):
    p = np.radians(pitch_deg)
    f = np.array([np.cos(p), -np.sin(p), 0.0])
    right = np.array([0.0, 0.0, 1.0])
    up = np.cross(right, f)
    t = np.tan(np.radians(fov_deg) / 2)
    u = (np.arange(side) + 0.5) / side * 2 - 1
    V, U = np.meshgrid(-u, u, indexing="ij")                 # row-major pixels, top row first
    d = f + (U * t)[..., None] * right + (V * t)[..., None] * up
    return RR.pack(np.asarray(eye, np.float32), d.reshape(-1, 3))


def workloads_for(half, top, rng):
    """the three families of N_RAYS rays over a footprint [-half, half]^2"""
    rand = RR.pack(np.c_[rng.uniform(-half, half, N_RAYS), rng.uniform(-5, 30, N_RAYS), rng.uniform(-half, half, N_RAYS)],
                   rng.normal(size=(N_RAYS, 3)))
    xz = rng.uniform(-0.9 * half, 0.9 * half, (N_RAYS, 2)).astype(np.float32)
    vert = RR.pack(np.c_[xz[:, 0], np.full(N_RAYS, top), xz[:, 1]], [0.0, -1.0, 0.0])
    return {"camera": camera_rays(1000, [0.0, 20.0, 0.0]), "random": rand, "vertical": vert}, xz


def bench_surface(o, name, R, half, vert, norm, white, wstride, a, stream, shim, rng):
    top = float(vert[:, 1].max()) + 10.0
    fams, xz = workloads_for(half, top, rng)
    d_out, d_hit = torch.empty((N_RAYS, 8), device="cuda"), torch.empty((N_RAYS, 2), dtype=torch.int32, device="cuda")
    d_one = torch.from_numpy(fams["vertical"][:1].copy()).cuda()
    rows = []
    for B in a.blocks:
        mw.set_switch("MW_RC_BLOCK", B)
        row = {"surface": name, "block": B}
        row["build_plus_one_ray_us"] = timed(stream, a.reps, lambda: o.raycast_device(d_one.data_ptr(), 1, d_out.data_ptr(), d_hit.data_ptr()))
        for fam, rays in fams.items():
            d_rays = torch.from_numpy(rays).cuda()
            row[fam + "_us"] = timed(stream, a.reps, lambda: o.raycast_device(d_rays.data_ptr(), N_RAYS, d_out.data_ptr(), d_hit.data_ptr()))
            if B == a.blocks[0]:
                row[fam + "_hit_fraction"] = round(float((d_hit[:, 0] >= 0).float().mean().item()), 4)
        rows.append(row)
    mw.set_switch("MW_RC_BLOCK", 0)
    d_xz, d_q = torch.from_numpy(xz).cuda(), torch.empty((N_RAYS, 8), device="cuda")
    q = {"surface": name, "query_surface_world_us": timed(stream, a.reps, lambda: o.query_surface_device(d_xz.data_ptr(), N_RAYS,
                                                                                                            d_q.data_ptr()))}
    torch.cuda.synchronize()
    # the shim's traversal on one host core, per 10^6 rays, over the tree the library builds by default (MW_RC_DEFAULT_BLOCK)
    m = RR.Mesh(R, vert, norm, white, wstride)
    DEFAULT_BLOCK = shim.rc_shim_default_block()
    q["cpu_block"] = DEFAULT_BLOCK
    box = np.empty((shim.rc_shim_nodes(R, DEFAULT_BLOCK), 8), np.float32)
    t0 = time.perf_counter()
    shim.rc_shim_build(R, RR._p(m.vert), DEFAULT_BLOCK, RR._p(box))
    q["cpu_build_us"] = round((time.perf_counter() - t0) * 1e6, 1)
    for fam, rays in fams.items():
        sub = np.ascontiguousarray(rays[rng.choice(N_RAYS, a.cpu_rays, replace=False)])
        out, hit = np.empty((len(sub), 8), np.float32), np.empty((len(sub), 2), np.int32)
        t0 = time.perf_counter()
        shim.rc_shim_trace(R, RR._p(m.vert), RR._p(m.norm), RR._p(m.white), wstride, DEFAULT_BLOCK, RR._p(box), RR._p(sub), len(sub), RR._p(out),
                           RR._p(hit))
        q["cpu_" + fam + "_us_per_1e6"] = round((time.perf_counter() - t0) * 1e6 * N_RAYS / len(sub), 1)
    rows.append(q)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--blocks", default="2,4,8,16")
    ap.add_argument("--cpu-rays", type=int, default=20000)
    a = ap.parse_args()
    a.blocks = [int(b) for b in a.blocks.split(",")]
    nat.require_product_build("raycast_bench")
    stream = torch.cuda.current_stream()
    shim = RR.build_shim(os.path.join(tempfile.mkdtemp(), "librc_shim.so"))
    rng = np.random.default_rng(2026)
    rows = []
    p = workloads.fftmesh_params(1024)
    o = mw.Ocean(resolution=1024, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                 choppiness=p.choppiness, gravity=p.gravity, device=0)
    o.set_stream(stream.cuda_stream)
    v, n, c = o.evaluate(2.0)
    rows += bench_surface(o, "fftmesh_1024", 1024, 512.0, v, n, c.reshape(-1), 4, a, stream, shim, rng)
    o.set_stream(None)
    o.close()
    r = mw.Ocean(resolution=128, length=434.48, wind=(14.45, 12.0), amplitude=0.41, choppiness=1.5, mult=1.5,
                 semantics=nat.MW_SEM_OCEANRENDERER, device=0)
    r.set_stream(stream.cuda_stream)
    r.generate_texture(1.0 / 60.0)
    v, n, c = r.displace_mesh()
    rows += bench_surface(r, "oceanrenderer_128", 128, 64.0, v, n, c, 1, a, stream, shim, rng)
    r.set_stream(None)
    r.close()
    print(json.dumps({"tool": "raycast_bench", "build": nat.build_id(), "device": torch.cuda.get_device_name(0), "rays": N_RAYS,
                      "rows": rows}))


if __name__ == "__main__":
    main()
