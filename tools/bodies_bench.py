"""Floating-bodies timing (mw_ocean_step_bodies_device) on the 1024^2 FFTMesh: one JSON line.  HIP events around back-to-back calls on
the handle's stream (torch's current stream), median of --reps.

  buoys   1024 icospheres (162 vertices, 320 triangles)
  boats   64 barges of 5600 triangles (3114 vertices)
  ship    1 barge of 99440 triangles (51054 vertices: its slab does not fit in LDS, so both forced plans run per substep)

each with 8 substeps, hydrostatic-only and with drag: the two forced plans (switch MW_BODIES_PLAN 0 and 1), the built-in rule (-1),
and 8 x mw_ocean_hull_forces_device as the caller-side baseline (forces only: no integration).  Every timed call starts from the same
state (a device copy before the call, timed with it; the copy alone is reported).

Usage: python tools/bodies_bench.py [--reps 50]"""
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
    return float(np.median(per)), float(np.min(per)), float(np.percentile(per, 90))


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
    ap.add_argument("--substeps", type=int, default=8)
    a = ap.parse_args()
    nat.require_product_build("bodies_bench")
    stream = torch.cuda.current_stream()
    p = workloads.fftmesh_params(1024)
    o = mw.Ocean(resolution=1024, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                 choppiness=p.choppiness, gravity=p.gravity, device=0)
    o.set_stream(stream.cuda_stream)
    o.evaluate(2.0)
    K, dt = a.substeps, 1.0 / 60
    rows = []
    for name, (hull0, tris), bodies in cases():
        m, c, I = mw.hull_mass_properties(hull0, tris, 500.0)
        hull = np.ascontiguousarray(hull0 - c, np.float32)
        nb, nv, nt = len(bodies), len(hull), len(tris)
        d_h, d_t = torch.from_numpy(hull).cuda(), torch.from_numpy(np.ascontiguousarray(tris)).cuda()
        d_b0 = torch.from_numpy(bodies).cuda()
        d_b = d_b0.clone()
        d_m = torch.from_numpy(mw.pack_mass(np.full(nb, m), np.broadcast_to(I, (nb, 3, 3)))).cuda()
        d_o = torch.empty((nb, 8), device="cuda")
        torch.cuda.synchronize()
        row = {"case": name, "nbodies": nb, "nverts": nv, "ntris": nt, "substeps": K,
               "copy_us_median": timed(stream, a.reps, lambda: d_b.copy_(d_b0))[0]}
        for mode, kw in (("hydro", {}), ("drag", dict(linear_drag=20.0, quadratic_drag=50.0))):
            def step():
                d_b.copy_(d_b0)
                o.step_bodies_device(d_h.data_ptr(), nv, d_t.data_ptr(), nt, d_b.data_ptr(), d_m.data_ptr(), nb, dt, K, d_o.data_ptr(), **kw)
            for plan in (0, 1, -1):
                mw.set_switch("MW_BODIES_PLAN", plan)
                t = timed(stream, a.reps, step)
                row["%s_plan%s_us" % (mode, {0: "0", 1: "1", -1: "_rule"}[plan])] = {"median": t[0], "min": t[1], "p90": t[2]}
            mw.set_switch("MW_BODIES_PLAN", -1)
            out = d_o.cpu().numpy()
            row["%s_finite_rows" % mode] = int(np.isfinite(out).all(1).sum())

            def forces():
                for _ in range(K):
                    o.hull_forces_device(d_h.data_ptr(), nv, d_t.data_ptr(), nt, d_b0.data_ptr(), nb, d_o.data_ptr(), **kw)
            t = timed(stream, a.reps, forces)
            row["%s_8x_hull_forces_us" % mode] = {"median": t[0], "min": t[1], "p90": t[2]}
        rows.append(row)
    o.set_stream(None)
    o.close()
    print(json.dumps({"tool": "bodies_bench", "build": nat.build_id(), "device": torch.cuda.get_device_name(0), "rows": rows}))


if __name__ == "__main__":
    main()
