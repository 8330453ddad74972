"""Draught (mw_ocean_set_draught) on the 1024^2 FFTMesh: what hull forces and 8 substeps of stepping cost with the hull family reading
the water column, beside the same calls with the switch off.  One JSON line, also written to profiles/draught_bench_<build id>.json.
HIP events around back-to-back device-form calls on the handle's stream (torch's current stream), median of --reps.

  buoys   1024 icospheres (162 vertices, 320 triangles)
  boats   64 barges of 5600 triangles (3114 vertices)
  ship    1 barge of 99440 triangles (51054 vertices)

with L = 4 layers at depths (0, 2, 4, 8) and L = 8 at (0, 2, 4, ..., 128); each case hydrostatic-only and with drag, draught off and on.
With draught on the layers are built by the first call after a frame and reused by the next ones, so the table has both: the call in
steady state (layers built) and the first call after a new frame; the layer build alone and the surface velocity field alone stand
beside them.  layers_located is the mean number of layers the vertex step walks per instance vertex (from mw_ocean_query_column's lambda).

Usage: python tools/draught_bench.py [--reps 50] [--substeps 8]"""
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


def timed(stream, reps, fn, before=None, warm=3):
    """median / min / p90 in microseconds of fn between two events; before() runs outside the timed region"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    per = []
    for k in range(warm + reps):
        if before:
            before()
        ev[0].record(stream)
        fn()
        ev[1].record(stream)
        ev[1].synchronize()
        if k >= warm:
            per.append(ev[0].elapsed_time(ev[1]) * 1e3)
    return {"median": float(np.median(per)), "min": float(np.min(per)), "p90": float(np.percentile(per, 90))}


def cases():
    rng = np.random.default_rng(1)

    def bodies(n, span, dy):
        p = np.stack([rng.uniform(-span, span, n), rng.uniform(-dy, dy, n), rng.uniform(-span, span, n)], 1)
        return mw.pack_bodies(p, H.random_quaternions(n, rng) * [0.1, 1, 0.1, 1], rng.standard_normal((n, 3)), 0.1 * rng.standard_normal((n, 3)))
    yield "buoys", H.icosphere(1.0), bodies(1024, 400.0, 0.5)
    yield "boats", H.grid_hull(25, 50, 6.0, 20.0, 2.0), bodies(64, 380.0, 1.0)
    yield "ship", H.grid_hull(110, 220, 40.0, 120.0, 8.0), bodies(1, 0.0, 1.0)


DRAG = dict(linear_drag=20.0, quadratic_drag=50.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--substeps", type=int, default=8)
    a = ap.parse_args()
    nat.require_product_build("draught_bench")
    stream = torch.cuda.current_stream()
    p = workloads.fftmesh_params(1024)
    o = mw.Ocean(resolution=1024, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                 choppiness=p.choppiness, gravity=p.gravity, device=0)
    o.set_stream(stream.cuda_stream)
    o.evaluate(2.0)
    K, dt = a.substeps, 1.0 / 60
    tick = [2.0]
    d_vel = torch.empty((1024 * 1024, 3), device="cuda")

    def new_frame():
        tick[0] += 0.125
        o.evaluate(tick[0])

    rows = [{"case": "velocity_field", "us": timed(stream, a.reps, lambda: o.velocity_device(d_vel.data_ptr()))}]
    all_cases = list(cases())
    for L in (4, 8):
        depths = np.concatenate([[0.0], 2.0 * 2.0 ** np.arange(L - 1)]).astype(np.float32)
        o.set_draught(False)
        o.set_column(depths)
        rows.append({"case": "build", "layers": L, "after_frame_us": timed(stream, a.reps, lambda: o.column_layers(1), before=new_frame)})
        for name, (hull0, tris), bodies in all_cases:
            m, c, I = mw.hull_mass_properties(hull0, tris, 500.0)
            hull = np.ascontiguousarray(hull0 - c, np.float32)
            nb, nv, nt = len(bodies), len(hull), len(tris)
            d_h, d_t = torch.from_numpy(hull).cuda(), torch.from_numpy(np.ascontiguousarray(tris)).cuda()
            d_b0 = torch.from_numpy(bodies).cuda()
            d_b = d_b0.clone()
            d_m = torch.from_numpy(mw.pack_mass(np.full(nb, m), np.broadcast_to(I, (nb, 3, 3)))).cuda()
            d_o = torch.empty((nb, 8), device="cuda")
            torch.cuda.synchronize()
            col = o.query_column(H.transform(bodies, hull).reshape(-1, 3))
            lam = col[:, 7]
            located = np.where(lam == np.floor(lam), lam + 1, np.floor(lam) + 2)   # on a layer: that layer and those above; between: one more
            located = np.where(col[:, 3] < 0, 1, np.minimum(located, L))            # in the air: the surface alone
            row = {"case": name, "layers": L, "nbodies": nb, "nverts": nv, "ntris": nt, "points": nb * nv, "substeps": K,
                   "layers_located": float(np.nanmean(located)), "copy_us": timed(stream, a.reps, lambda: d_b.copy_(d_b0))}

            def forces(kw):
                return lambda: o.hull_forces_device(d_h.data_ptr(), nv, d_t.data_ptr(), nt, d_b0.data_ptr(), nb, d_o.data_ptr(), **kw)

            def step(kw):
                def f():
                    d_b.copy_(d_b0)
                    o.step_bodies_device(d_h.data_ptr(), nv, d_t.data_ptr(), nt, d_b.data_ptr(), d_m.data_ptr(), nb, dt, K, d_o.data_ptr(), **kw)
                return f

            for draught in (False, True):
                o.set_draught(draught)
                tag = "on" if draught else "off"
                for mode, kw in (("hydro", {}), ("drag", DRAG)):
                    row["forces_%s_%s_us" % (mode, tag)] = timed(stream, a.reps, forces(kw))
                    out = d_o.cpu().numpy()
                    row["forces_%s_%s_finite_rows" % (mode, tag)] = int(np.isfinite(out).all(1).sum())
                    row["step_%s_%s_us" % (mode, tag)] = timed(stream, a.reps, step(kw))
                    if draught:
                        row["forces_%s_on_after_frame_us" % mode] = timed(stream, a.reps, forces(kw), before=new_frame)
                        row["step_%s_on_after_frame_us" % mode] = timed(stream, a.reps, step(kw), before=new_frame)
            o.set_draught(False)
            rows.append(row)
    o.set_stream(None)
    o.close()
    line = json.dumps({"tool": "draught_bench", "build": nat.build_id(), "device": torch.cuda.get_device_name(0), "rows": rows})
    print(line)
    path = os.path.join(REPO, "profiles", "draught_bench_%s.json" % nat.build_id().split(" ")[0])
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
