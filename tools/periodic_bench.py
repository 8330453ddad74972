"""The periodic surface (mw_ocean_set_periodic) on the 1024^2 FFTMesh: what the tiled services cost next to the one-footprint ones.
HIP events around back-to-back device-form calls on the handle's stream (torch's current stream), median of --reps.  Prints one JSON line
and writes it to profiles/periodic_bench_<build id>.json.

  queries  10^6 world-mode points inside the footprint with the switch off; the same points with it on; 10^6 points spread over 7 x 7 tiles
  hulls    mw_ocean_hull_forces_device, 1024 icospheres (162 vertices, 320 triangles), hydrostatic and with drag, off and on
  bodies   mw_ocean_step_bodies_device on the same fleet, 8 substeps, the built-in plan, off and on

The off rows are the cases of tools/query_bench.py, tools/hull_bench.py and tools/bodies_bench.py.
usage: python tools/periodic_bench.py [--reps R]"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mistral-water_amd"), os.path.join(REPO, "tests")]
import torch  # noqa: E402  (initialises its HIP runtime before the library)
torch.cuda.init()
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
    return {"median": float(np.median(per)), "min": float(np.min(per)), "p90": float(np.percentile(per, 90))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    nat.require_product_build("periodic_bench")
    stream = torch.cuda.current_stream()
    p = workloads.fftmesh_params(1024)
    o = mw.Ocean(resolution=1024, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                 choppiness=p.choppiness, gravity=p.gravity, device=0)
    o.set_stream(stream.cuda_stream)
    vert = o.evaluate(2.0)[0]
    P, uw = o.period, p.unit_width
    x0 = (0 - 512) * uw + uw / 2
    rest = x0 + uw * np.arange(1024)
    dmax = float(np.abs(vert[:, [0, 2]] - np.stack(np.meshgrid(rest, rest, indexing="ij"), -1).reshape(-1, 2)).max())
    n = 1000000
    rng = np.random.default_rng(n)
    inside = rng.uniform(rest[0] + dmax, rest[-1] - dmax, (n, 2)).astype(np.float32)
    spread = rng.uniform(x0 - 3 * P, x0 + 4 * P, (n, 2)).astype(np.float32)
    d_out = torch.empty((n, 8), device="cuda")
    d_vout = torch.empty((n, 4), device="cuda")
    rows = []

    def query_rows(label, xz, on):
        o.set_periodic(on)
        d_xz = torch.from_numpy(xz).cuda()
        torch.cuda.synchronize()
        t = timed(stream, a.reps, lambda: o.query_surface_device(d_xz.data_ptr(), n, d_out.data_ptr(), mode="world"))
        out = d_out.cpu().numpy()
        tv = timed(stream, a.reps, lambda: o.query_velocity_device(d_xz.data_ptr(), n, d_vout.data_ptr(), mode="world"))
        rows.append({"case": "query_world", "points": label, "periodic": on, "n": n, "surface_us": t, "velocity_us": tv,
                     "resolved_fraction": float(np.mean(out[:, 7] <= 1e-4 * uw))})
    query_rows("inside", inside, False)
    query_rows("inside", inside, True)
    query_rows("7x7_tiles", spread, True)

    # the fleet of tools/hull_bench.py / tools/bodies_bench.py: 1024 icospheres over the footprint; on, the same fleet over 7 x 7 tiles too
    hull0, tris = H.icosphere(1.0)
    m, c, I = mw.hull_mass_properties(hull0, tris, 500.0)
    hull = np.ascontiguousarray(hull0 - c, np.float32)
    nb, nv, nt = 1024, len(hull), len(tris)
    frng = np.random.default_rng(1)
    pos = np.stack([frng.uniform(-400, 400, nb), frng.uniform(-0.5, 0.5, nb), frng.uniform(-400, 400, nb)], 1)
    quat = H.random_quaternions(nb, frng) * [0.1, 1, 0.1, 1]
    vel, ang = frng.standard_normal((nb, 3)), 0.1 * frng.standard_normal((nb, 3))
    tiles = frng.integers(-3, 4, (nb, 3)) * [1, 0, 1]
    d_h, d_t = torch.from_numpy(hull).cuda(), torch.from_numpy(np.ascontiguousarray(tris)).cuda()
    d_m = torch.from_numpy(mw.pack_mass(np.full(nb, m), np.broadcast_to(I, (nb, 3, 3)))).cuda()
    d_o = torch.empty((nb, 8), device="cuda")
    K, dt = 8, 1.0 / 60
    for label, on, shift in (("inside", False, 0), ("inside", True, 0), ("7x7_tiles", True, 1)):
        o.set_periodic(on)
        d_b0 = torch.from_numpy(mw.pack_bodies(pos + shift * tiles * P, quat, vel, ang)).cuda()
        d_b = d_b0.clone()
        torch.cuda.synchronize()
        for mode, kw in (("hydro", {}), ("drag", dict(linear_drag=20.0, quadratic_drag=50.0))):
            def forces():
                o.hull_forces_device(d_h.data_ptr(), nv, d_t.data_ptr(), nt, d_b0.data_ptr(), nb, d_o.data_ptr(), **kw)

            def step():
                d_b.copy_(d_b0)
                o.step_bodies_device(d_h.data_ptr(), nv, d_t.data_ptr(), nt, d_b.data_ptr(), d_m.data_ptr(), nb, dt, K, d_o.data_ptr(), **kw)
            tf = timed(stream, a.reps, forces)
            ts = timed(stream, a.reps, step)
            out = d_o.cpu().numpy()
            rows.append({"case": "fleet_" + mode, "points": label, "periodic": on, "nbodies": nb, "nverts": nv, "ntris": nt, "substeps": K,
                         "hull_forces_us": tf, "step_bodies_us": ts, "finite_rows": int(np.isfinite(out).all(1).sum()),
                         "max_residual": float(np.nanmax(out[:, 7]))})
    o.set_periodic(False)
    o.set_stream(None)
    o.close()
    line = json.dumps({"tool": "periodic_bench", "build": nat.build_id(), "device": torch.cuda.get_device_name(0), "period": P, "rows": rows})
    print(line)
    path = os.path.join(REPO, "profiles", "periodic_bench_%s.json" % nat.build_id().split(" ")[0])
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
