"""Mixed-fleet timing (mw_ocean_fleet_forces_device, mw_ocean_step_fleet_device) on the 1024^2 FFTMesh against the single-hull calls that
do the same work: one JSON line, printed and written to profiles/fleet_bench_<build id>.json.  HIP events around each call sequence on
the handle's stream (torch's current stream); within a case the fleet call and its baseline alternate rep by rep, so both see the same
clocks; median, min and p90 of --reps.

  a  scene      1024 icospheres, 64 barges of 5600 triangles and the 99440-triangle hull in one call, against the three single-hull calls
  b  shapes     32 shapes of 32 small bodies each, against 32 single-hull calls
  c  one_hull   1024 icospheres as a one-hull fleet against the existing call, and the existing call against itself (run-to-run spread)

each as forces (one call) and as a step of 8 substeps, hydrostatic-only and with drag.  Every timed step starts from the same state (a
device copy before the call, timed with it).

Usage: python tools/fleet_bench.py [--reps 50]"""
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


def timed_alternating(stream, reps, fns):
    """{name: (median, min, p90) in us} of the callables of `fns`, run one after the other in every rep"""
    for _ in range(3):
        for fn in fns.values():
            fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    per = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ev[0].record(stream)
            fn()
            ev[1].record(stream)
            ev[1].synchronize()
            per[k].append(ev[0].elapsed_time(ev[1]) * 1e3)
    return {k: {"median": float(np.median(v)), "min": float(np.min(v)), "p90": float(np.percentile(v, 90))} for k, v in per.items()}


def scenes():
    rng = np.random.default_rng(1)

    def bodies(n, span, dy):
        p = np.stack([rng.uniform(-span, span, n), rng.uniform(-dy, dy, n), rng.uniform(-span, span, n)], 1)
        return mw.pack_bodies(p, H.random_quaternions(n, rng) * [0.1, 1, 0.1, 1], rng.standard_normal((n, 3)), 0.1 * rng.standard_normal((n, 3)))
    buoys = (H.icosphere(1.0), bodies(1024, 400.0, 0.5))
    yield "a_scene", [buoys, (H.grid_hull(25, 50, 6.0, 20.0, 2.0), bodies(64, 380.0, 1.0)),
                      (H.grid_hull(110, 220, 40.0, 120.0, 8.0), bodies(1, 0.0, 1.0))]
    shapes = []
    for k in range(32):  # boxes, icospheres of 80 and 320 triangles and small barges, every one its own size
        s = 0.6 + 0.05 * k
        hull = (H.box(2 * s, s, 3 * s), H.icosphere(s, 1), H.icosphere(s, 2), H.grid_hull(4, 6, 2 * s, 3 * s, 0.5 * s))[k % 4]
        shapes.append((hull, bodies(32, 400.0, 0.3)))
    yield "b_shapes", shapes
    yield "c_one_hull", [buoys]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--substeps", type=int, default=8)
    a = ap.parse_args()
    if a.reps < 30:
        ap.error("--reps must be at least 30")
    nat.require_product_build("fleet_bench")
    stream = torch.cuda.current_stream()
    p = workloads.fftmesh_params(1024)
    o = mw.Ocean(resolution=1024, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                 choppiness=p.choppiness, gravity=p.gravity, device=0)
    o.set_stream(stream.cuda_stream)
    o.evaluate(2.0)
    K, dt = a.substeps, 1.0 / 60
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    rows = []
    for name, scene in scenes():
        hulls, masses, allb = [], [], []
        for (hull0, tris), b in scene:
            m, c, I = mw.hull_mass_properties(hull0, tris, 500.0)
            hulls.append((np.ascontiguousarray(hull0 - c, np.float32), tris, len(b)))
            masses.append(mw.pack_mass(np.full(len(b), m), np.broadcast_to(I, (len(b), 3, 3))))
            allb.append(b)
        x, t, table = mw.pack_fleet(hulls)
        n = int(table[:, 4].sum())
        d_x, d_t, d_b0, d_m = up(x), up(t), up(np.concatenate(allb)), up(np.concatenate(masses))
        d_b, d_o, d_o1 = d_b0.clone(), torch.empty((n, 8), device="cuda"), torch.empty((n, 8), device="cuda")
        first = np.concatenate([[0], np.cumsum(table[:, 4])])
        torch.cuda.synchronize()

        def ptr(tensor, row, width):  # the device address of row `row` of a [*, width] float32 / int32 tensor
            return tensor.data_ptr() + 4 * width * int(row)

        row = {"case": name, "nhulls": len(hulls), "total_bodies": n, "total_verts": len(x), "total_tris": len(t), "substeps": K}
        for mode, cf in (("hydro", [1000.0, 9.81, 0.0, 0.0, np.nan]), ("drag", [1000.0, 9.81, 20.0, 50.0, np.nan])):
            kw = dict(linear_drag=cf[2], quadratic_drag=cf[3])

            def fleet_forces():
                o.fleet_forces_device(d_x.data_ptr(), len(x), d_t.data_ptr(), len(t), table, d_b0.data_ptr(), n, d_o.data_ptr(), coeffs=cf)

            def single_forces():
                for h, (vf, nv, tf, nt, nb) in enumerate(table):
                    o.hull_forces_device(ptr(d_x, vf, 3), int(nv), ptr(d_t, tf, 3), int(nt), ptr(d_b0, first[h], 16), int(nb),
                                         ptr(d_o1, first[h], 8), **kw)

            def fleet_step():
                d_b.copy_(d_b0)
                o.step_fleet_device(d_x.data_ptr(), len(x), d_t.data_ptr(), len(t), table, d_b.data_ptr(), d_m.data_ptr(), n, dt, K,
                                    d_out=d_o.data_ptr(), coeffs=cf)

            def single_step():
                d_b.copy_(d_b0)
                for h, (vf, nv, tf, nt, nb) in enumerate(table):
                    o.step_bodies_device(ptr(d_x, vf, 3), int(nv), ptr(d_t, tf, 3), int(nt), ptr(d_b, first[h], 16), ptr(d_m, first[h], 8),
                                         int(nb), dt, K, ptr(d_o1, first[h], 8), **kw)
            fns = {"fleet_forces": fleet_forces, "single_forces": single_forces, "fleet_step": fleet_step, "single_step": single_step}
            if name == "c_one_hull":  # the existing call twice in the same run: its run-to-run spread
                fns.update(single_forces_again=single_forces, single_step_again=single_step)
            t_us = timed_alternating(stream, a.reps, fns)
            fleet_step()
            fb, fo = d_b.cpu().numpy().copy(), d_o.cpu().numpy().copy()
            single_step()
            sb, so = d_b.cpu().numpy(), d_o1.cpu().numpy()
            row[mode] = dict(t_us, finite_rows=int(np.isfinite(fo).all(1).sum()),
                             same_bits=bool(np.array_equal(fb.view(np.uint32), sb.view(np.uint32)) and
                                            np.array_equal(fo.view(np.uint32), so.view(np.uint32))),
                             forces_ratio=t_us["fleet_forces"]["median"] / t_us["single_forces"]["median"],
                             step_ratio=t_us["fleet_step"]["median"] / t_us["single_step"]["median"])
            if name == "c_one_hull":
                row[mode].update(forces_spread=t_us["single_forces_again"]["median"] / t_us["single_forces"]["median"],
                                 step_spread=t_us["single_step_again"]["median"] / t_us["single_step"]["median"])
        rows.append(row)
    o.set_stream(None)
    o.close()
    line = json.dumps({"tool": "fleet_bench", "build": nat.build_id(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows})
    print(line)
    path = os.path.join(REPO, "profiles", "fleet_bench_%s.json" % nat.build_id().split(" ")[0])
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
