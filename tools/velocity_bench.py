"""Surface velocity timing (mw_ocean_velocity_device / mw_ocean_query_velocity_device) against the frame and the surface query it
rides on: one JSON line.  HIP events around back-to-back calls on the handle's stream (torch's current stream), median of --reps.

  fftmesh_1024       velocity_device (spectrum already weighted) vs one single-step evaluate_device frame
  oceanrenderer_128  velocity_device vs one generate_texture_device frame (1024^2 textures)
  queries            10^3 / 10^6 world- and rest-mode query_velocity_device vs query_surface_device on the 1024^2 FFTMesh

Usage: python tools/velocity_bench.py [--reps 50]"""
import argparse
import ctypes as C
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mistral-water_amd"), os.path.join(REPO, "tests")]
import torch  # noqa: E402  (initialises its HIP runtime before the library)

import numpy as np  # noqa: E402
import mistral_water as mw  # noqa: E402
from mistral_water import _native as nat  # noqa: E402
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    nat.require_product_build("velocity_bench")
    stream = torch.cuda.current_stream()
    rows = []
    p = workloads.fftmesh_params(1024)
    o = mw.Ocean(resolution=1024, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                 choppiness=p.choppiness, gravity=p.gravity, device=0)
    o.set_stream(stream.cuda_stream)
    vert = o.evaluate(2.0)[0]
    NN = 1024 * 1024
    d_vel = torch.empty((NN, 3), device="cuda")
    d_v, d_n, d_w = torch.empty((NN, 3), device="cuda"), torch.empty((NN, 3), device="cuda"), torch.empty((NN,), device="cuda")
    t = (C.c_float * 1)(2.0)
    frame = lambda: nat.check(nat.lib().mw_ocean_evaluate_device(o._h, t, 1, C.c_void_p(d_v.data_ptr()), C.c_void_p(d_n.data_ptr()),  # noqa: E731
                                                                 C.c_void_p(d_w.data_ptr()), 0))
    vel = lambda: o.velocity_device(d_vel.data_ptr())  # noqa: E731
    fm, fmin = timed(stream, a.reps, frame)
    vm, vmin = timed(stream, a.reps, vel)
    rows.append({"workload": "fftmesh_1024", "velocity_us_median": vm, "velocity_us_min": vmin, "frame_us_median": fm, "frame_us_min": fmin})
    rc = np.asarray([(a_ - 512) * p.unit_width + p.unit_width / 2 for a_ in range(1024)], np.float32)
    dmax = float(np.abs(vert[:, 0] - np.repeat(rc, 1024)).max())
    for n in (1000, 1000000):
        xz = np.random.default_rng(n).uniform(rc[0] + dmax, rc[-1] - dmax, (n, 2)).astype(np.float32)
        d_xz = torch.from_numpy(xz).cuda()
        d_out4, d_out8 = torch.empty((n, 4), device="cuda"), torch.empty((n, 8), device="cuda")
        for mode in ("rest", "world"):
            qv = timed(stream, a.reps, lambda: o.query_velocity_device(d_xz.data_ptr(), n, d_out4.data_ptr(), mode=mode))
            qs = timed(stream, a.reps, lambda: o.query_surface_device(d_xz.data_ptr(), n, d_out8.data_ptr(), mode=mode))
            rows.append({"workload": "fftmesh_1024_query", "n": n, "mode": mode, "query_velocity_us_median": qv[0],
                         "query_surface_us_median": qs[0], "ratio": qv[0] / qs[0]})
    o.set_stream(None)
    o.close()
    r = mw.Ocean(resolution=128, length=434.48, wind=(14.45, 12.0), amplitude=0.41, choppiness=1.5, mult=1.5,
                 semantics=nat.MW_SEM_OCEANRENDERER, device=0)
    r.set_stream(stream.cuda_stream)
    r.generate_texture(1.0 / 60.0)
    d_rv = torch.empty((128 * 128, 3), device="cuda")
    fm, _ = timed(stream, a.reps, lambda: nat.check(nat.lib().mw_ocean_generate_texture_device(r._h, C.c_float(1.0 / 60.0), None, None,
                                                                                                None, None)))
    vm, vmin = timed(stream, a.reps, lambda: r.velocity_device(d_rv.data_ptr()))
    rows.append({"workload": "oceanrenderer_128", "velocity_us_median": vm, "velocity_us_min": vmin, "frame_us_median": fm})
    r.set_stream(None)
    r.close()
    print(json.dumps({"tool": "velocity_bench", "build": nat.build_id(), "device": torch.cuda.get_device_name(0), "rows": rows}))


if __name__ == "__main__":
    main()
