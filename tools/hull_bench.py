"""Hull-forces timing (mw_ocean_hull_forces_device) on the 1024^2 FFTMesh against a world-mode query_surface_device of the same
nbodies * nverts points: one JSON line.  HIP events around back-to-back calls on the handle's stream (torch's current stream), median of
--reps.

  buoys   1024 icospheres (162 vertices, 320 triangles)
  boats   64 barges of 5600 triangles (3114 vertices)
  ship    1 barge of 99440 triangles (51054 vertices)

each hydrostatic-only (no velocity field) and with drag (the velocity field is computed in the call), and the query of the instance
vertices' (x, z).

Usage: python tools/hull_bench.py [--reps 50]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mistral-water_amd"), os.path.join(REPO, "tests")]
import torch  # noqa: E402  (initialises its HIP runtime before the library)

import numpy as np  # noqa: E402
import mistral_water as mw  # noqa: E402
from mistral_water import _native as nat  # noqa: E402
import hull_ref as H  # noqa: E402
import workloads  # noqa: E402


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
    return float(np.median(per)), float(np.min(per))


def cases():
    rng = np.random.default_rng(1)

    def bodies(n, span, dy):
        p = np.stack([rng.uniform(-span, span, n), rng.uniform(-dy, dy, n), rng.uniform(-span, span, n)], 1)
        return mw.pack_bodies(p, H.random_quaternions(n, rng) * [0.1, 1, 0.1, 1], rng.standard_normal((n, 3)), 0.1 * rng.standard_normal((n, 3)))
    yield "buoys", H.icosphere(1.0), bodies(1024, 400.0, 0.5)
    yield "boats", H.grid_hull(25, 50, 6.0, 20.0, 2.0), bodies(64, 380.0, 1.0)
    yield "ship", H.grid_hull(110, 220, 40.0, 120.0, 8.0), bodies(1, 0.0, 1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    nat.require_product_build("hull_bench")
    stream = torch.cuda.current_stream()
    p = workloads.fftmesh_params(1024)
    o = mw.Ocean(resolution=1024, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                 choppiness=p.choppiness, gravity=p.gravity, device=0)
    o.set_stream(stream.cuda_stream)
    o.evaluate(2.0)
    rows = []
    for name, (hull, tris), bodies in cases():
        nb, nv, nt = len(bodies), len(hull), len(tris)
        d_h, d_t, d_b = torch.from_numpy(hull).cuda(), torch.from_numpy(np.ascontiguousarray(tris)).cuda(), torch.from_numpy(bodies).cuda()
        d_o = torch.empty((nb, 8), device="cuda")
        x = H.transform(bodies, hull).reshape(-1, 3)
        d_xz = torch.from_numpy(np.ascontiguousarray(x[:, [0, 2]], np.float32)).cuda()
        d_q = torch.empty((nb * nv, 8), device="cuda")
        torch.cuda.synchronize()
        hydro = timed(stream, a.reps, lambda: o.hull_forces_device(d_h.data_ptr(), nv, d_t.data_ptr(), nt, d_b.data_ptr(), nb, d_o.data_ptr()))
        out = d_o.cpu().numpy()
        drag = timed(stream, a.reps, lambda: o.hull_forces_device(d_h.data_ptr(), nv, d_t.data_ptr(), nt, d_b.data_ptr(), nb, d_o.data_ptr(),
                                                                  linear_drag=20.0, quadratic_drag=50.0))
        query = timed(stream, a.reps, lambda: o.query_surface_device(d_xz.data_ptr(), nb * nv, d_q.data_ptr(), mode="world"))
        rows.append({"case": name, "nbodies": nb, "nverts": nv, "ntris": nt, "points": nb * nv,
                     "hydro_us_median": hydro[0], "hydro_us_min": hydro[1], "drag_us_median": drag[0], "drag_us_min": drag[1],
                     "query_surface_us_median": query[0], "hydro_over_query": hydro[0] / query[0],
                     "wet_bodies": int((out[:, 3] > 0).sum()), "max_residual": float(np.nanmax(out[:, 7])), "finite": bool(np.isfinite(out).all())})
    o.set_stream(None)
    o.close()
    print(json.dumps({"tool": "hull_bench", "build": nat.build_id(), "device": torch.cuda.get_device_name(0), "rows": rows}))


if __name__ == "__main__":
    main()
