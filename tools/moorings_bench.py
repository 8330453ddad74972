"""Moorings timing (mw_ocean_step_moored_device) on the 1024^2 FFTMesh beside mw_ocean_step_bodies_device on the same bodies in the same
process: one JSON line, printed and written to profiles/moorings_bench_<build id>.json.  HIP events around back-to-back calls on the
handle's stream (torch's current stream), median of --reps; the two calls alternate case by case, each after three warm-up calls.

  buoys   1024 icospheres (162 vertices, 320 triangles), 1 and 8 lines per body
  boats   64 barges of 5600 triangles (3114 vertices), 4 lines per body

each with 8 substeps, hydrostatic-only and with drag, on the periodic handle (the one-launch plan for the buoys, per substep for the
barges) and on the one footprint (always per substep).  Every line is taut: each body hangs on anchors 8 to 12 below and around it.
Every timed call starts from the same state (a device copy before the call, timed with it; the copy alone is reported).

Usage: python tools/moorings_bench.py [--reps 50]"""
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
from bodies_bench import timed  # noqa: E402


def cases():
    rng = np.random.default_rng(1)

    def bodies(n, span, dy):
        p = np.stack([rng.uniform(-span, span, n), rng.uniform(-dy, dy, n), rng.uniform(-span, span, n)], 1)
        return mw.pack_bodies(p, H.random_quaternions(n, rng) * [0.1, 1, 0.1, 1], rng.standard_normal((n, 3)), 0.1 * rng.standard_normal((n, 3)))
    buoys = bodies(1024, 400.0, 0.5)
    yield "buoys", H.icosphere(1.0), buoys, 1
    yield "buoys", H.icosphere(1.0), buoys, 8
    yield "boats", H.grid_hull(25, 50, 6.0, 20.0, 2.0), bodies(64, 380.0, 1.0), 4


def lines_for(bodies, K, m, rng):
    """K taut lines per body: anchors 8 to 12 away, below and around; stiffness and damping sized by the body's mass (h omega < 0.1)"""
    n = len(bodies)
    u = rng.standard_normal((n, K, 3))
    u[:, :, 1] = -1.0 - np.abs(u[:, :, 1])
    u /= np.linalg.norm(u, axis=2, keepdims=True)
    dist = rng.uniform(8.0, 12.0, (n, K))
    return mw.pack_lines(n, K, attach=rng.uniform(-0.5, 0.5, (n, K, 3)), anchor=bodies[:, None, 0:3] + u * dist[:, :, None],
                         rest_length=0.8 * dist, stiffness=2.0 * m, damping=0.5 * m)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--substeps", type=int, default=8)
    a = ap.parse_args()
    nat.require_product_build("moorings_bench")
    stream = torch.cuda.current_stream()
    p = workloads.fftmesh_params(1024)
    o = mw.Ocean(resolution=1024, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                 choppiness=p.choppiness, gravity=p.gravity, device=0)
    o.set_stream(stream.cuda_stream)
    o.evaluate(2.0)
    K, dt = a.substeps, 1.0 / 60
    rng = np.random.default_rng(2)
    rows = []
    for name, (hull0, tris), bodies, nl in cases():
        m, c, I = mw.hull_mass_properties(hull0, tris, 500.0)
        hull = np.ascontiguousarray(hull0 - c, np.float32)
        nb, nv, nt = len(bodies), len(hull), len(tris)
        d_h, d_t = torch.from_numpy(hull).cuda(), torch.from_numpy(np.ascontiguousarray(tris)).cuda()
        d_b0 = torch.from_numpy(bodies).cuda()
        d_b = d_b0.clone()
        d_m = torch.from_numpy(mw.pack_mass(np.full(nb, m), np.broadcast_to(I, (nb, 3, 3)))).cuda()
        d_l = torch.from_numpy(lines_for(bodies, nl, m, rng)).cuda()
        d_o, d_n = torch.empty((nb, 8), device="cuda"), torch.empty((nb, nl), device="cuda")
        torch.cuda.synchronize()
        for periodic in (True, False):
            o.set_periodic(periodic)
            row = {"case": name, "nbodies": nb, "nverts": nv, "ntris": nt, "substeps": K, "lines_per_body": nl, "periodic": periodic,
                   "copy_us_median": timed(stream, a.reps, lambda: d_b.copy_(d_b0))[0]}
            for mode, kw in (("hydro", {}), ("drag", dict(linear_drag=20.0, quadratic_drag=50.0))):
                def bodies_call():
                    d_b.copy_(d_b0)
                    o.step_bodies_device(d_h.data_ptr(), nv, d_t.data_ptr(), nt, d_b.data_ptr(), d_m.data_ptr(), nb, dt, K, d_o.data_ptr(), **kw)

                def moored_call():
                    d_b.copy_(d_b0)
                    o.step_moored_device(d_h.data_ptr(), nv, d_t.data_ptr(), nt, d_b.data_ptr(), d_m.data_ptr(), d_l.data_ptr(), nl, nb, dt, K,
                                         d_out=d_o.data_ptr(), d_tension=d_n.data_ptr(), **kw)
                tb = timed(stream, a.reps, bodies_call)
                tm = timed(stream, a.reps, moored_call)
                row["%s_step_bodies_us" % mode] = {"median": tb[0], "min": tb[1], "p90": tb[2]}
                row["%s_step_moored_us" % mode] = {"median": tm[0], "min": tm[1], "p90": tm[2]}
                row["%s_ratio" % mode] = tm[0] / tb[0]
                row["%s_finite_rows" % mode] = int(np.isfinite(d_o.cpu().numpy()).all(1).sum())
                row["%s_taut_lines" % mode] = int((d_n.cpu().numpy() > 0).sum())
            rows.append(row)
    o.set_periodic(False)
    o.set_stream(None)
    o.close()
    line = json.dumps({"tool": "moorings_bench", "build": nat.build_id(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows})
    print(line)
    path = os.path.join(REPO, "profiles", "moorings_bench_%s.json" % nat.build_id().split(" ")[0])
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
