"""Tiled raycast timing (mw_ocean_raycast_tiled_device) on the 1024^2 FFTMesh: one JSON line.  HIP events around back-to-back calls on
the handle's stream (torch's current stream), median, min and p90 of --reps.

  inside     10^6 camera, random and vertical rays of tools/raycast_bench.py inside the base footprint, next to mw_ocean_raycast_device on
             the same rays in the same run (that kernel is the yardstick: this change leaves it alone) and their ratio
  horizon    10^6 rays of a 1000 x 1000 camera 2 m above the sea looking at the horizon (90 degrees across, pitched 2 degrees down) at
             reach 16: time, hit share, out-of-reach share
  far        the same rays with the eye 1000 tiles out on both axes
  build+1    one call with a single ray: the hierarchy's launches plus one lane

A family is first timed on its first 2^16 rays; its full launch is skipped (and said so) if that predicts more than --max-seconds.

Usage: python tools/raycast_tiled_bench.py [--reps 20] [--reach 16]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mistral-water_amd"), os.path.join(REPO, "tests"), os.path.join(REPO, "tools")]
import torch  # noqa: E402  (initialises its HIP runtime before the library)

import numpy as np  # noqa: E402
import mistral_water as mw  # noqa: E402
from mistral_water import _native as nat  # noqa: E402
import workloads  # noqa: E402
from raycast_bench import N_RAYS, camera_rays, workloads_for  # noqa: E402

SUB = 1 << 16


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
    return {"median": round(float(np.median(per)), 1), "min": round(float(np.min(per)), 1), "p90": round(float(np.percentile(per, 90)), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--reach", type=int, default=nat.MW_RC_DEFAULT_REACH)
    ap.add_argument("--max-seconds", type=float, default=1.0)
    a = ap.parse_args()
    nat.require_product_build("raycast_tiled_bench")
    stream = torch.cuda.current_stream()
    rng = np.random.default_rng(2026)
    p = workloads.fftmesh_params(1024)
    o = mw.Ocean(resolution=1024, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                 choppiness=p.choppiness, gravity=p.gravity, device=0)
    o.set_stream(stream.cuda_stream)
    v, _, _ = o.evaluate(2.0)
    P = o.period
    d_out = torch.empty((N_RAYS, 8), device="cuda")
    d_hit2, d_hit4 = torch.empty((N_RAYS, 2), dtype=torch.int32, device="cuda"), torch.empty((N_RAYS, 4), dtype=torch.int32, device="cuda")

    def tiled(d_rays, n, reach):
        return lambda: o.raycast_tiled_device(d_rays.data_ptr(), n, d_out.data_ptr(), d_hit4.data_ptr(), reach=reach)

    def family(rays, reach):
        """the tiled cast of one family: the 2^16-ray probe, then the whole launch unless the probe predicts too long a kernel"""
        d_rays = torch.from_numpy(np.ascontiguousarray(rays)).cuda()
        row = {"reach": reach, "probe_65536_us": timed(stream, 5, tiled(d_rays, SUB, reach))}
        if row["probe_65536_us"]["median"] * 1e-6 * N_RAYS / SUB > a.max_seconds:
            row["skipped"] = "the probe predicts more than %g s per launch" % a.max_seconds
            return row, d_rays
        row["tiled_us"] = timed(stream, a.reps, tiled(d_rays, N_RAYS, reach))
        torch.cuda.synchronize()
        row["hit_fraction"] = round(float((d_hit4[:, 0] >= 0).float().mean().item()), 4)
        row["out_of_reach_fraction"] = round(float((d_hit4[:, 0] == -2).float().mean().item()), 4)
        return row, d_rays

    rows = []
    fams, _ = workloads_for(512.0, float(v[:, 1].max()) + 10.0, rng)
    for name, rays in fams.items():                                             # (a) inside the base footprint
        row, d_rays = family(rays, a.reach)
        row = {"case": "inside", "family": name, **row}
        row["untiled_us"] = timed(stream, a.reps, lambda: o.raycast_device(d_rays.data_ptr(), N_RAYS, d_out.data_ptr(), d_hit2.data_ptr()))
        torch.cuda.synchronize()
        row["untiled_hit_fraction"] = round(float((d_hit2[:, 0] >= 0).float().mean().item()), 4)
        if "tiled_us" in row:
            row["tiled_over_untiled"] = round(row["tiled_us"]["median"] / row["untiled_us"]["median"], 2)
        rows.append(row)
    horizon = camera_rays(1000, [0.0, float(v[:, 1].max()) + 2.0, 0.0], pitch_deg=2.0)
    rows.append({"case": "horizon", **family(horizon, a.reach)[0]})           # (b)
    far = horizon.copy()
    far[:, [0, 2]] += np.float32(1000.0 * P)
    rows.append({"case": "horizon_1000_tiles_out", **family(far, a.reach)[0]})  # (c)
    d_one = torch.from_numpy(fams["vertical"][:1].copy()).cuda()
    rows.append({"case": "build_plus_one_ray", "reach": a.reach, "tiled_us": timed(stream, a.reps, tiled(d_one, 1, a.reach)),   # (d)
                 "untiled_us": timed(stream, a.reps, lambda: o.raycast_device(d_one.data_ptr(), 1, d_out.data_ptr(), d_hit2.data_ptr()))})
    o.set_stream(None)
    o.close()
    print(json.dumps({"tool": "raycast_tiled_bench", "build": nat.build_id(), "device": torch.cuda.get_device_name(0), "rays": N_RAYS,
                      "period": P, "reps": a.reps, "rows": rows}))


if __name__ == "__main__":
    main()
