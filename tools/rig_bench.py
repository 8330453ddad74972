"""Rigged-fleet timing (mw_ocean_step_rigged_device) on the 1024^2 FFTMesh beside mw_ocean_step_fleet_device on the same scene in the same
run: one JSON line, printed and written to profiles/rig_bench_<build id>.json.  HIP events around each call on the handle's stream
(torch's current stream); within a case the two calls alternate rep by rep, so both see the same clocks; median, min and p90 of --reps.

The scene is fleet_bench's: 1024 icospheres (buoys), 64 barges of 5600 triangles and the one 99440-triangle hull, 8 substeps,
hydrostatic-only, on the periodic handle and on the one footprint, in three configurations:

  a_anchored  every body on one taut anchor line (K = 1)
  b_towed     the barges in 8 chains of 8, each barge tied to the one before it by a mirrored tow line, behind the first of its
              chain; the buoys and the big hull moored on one anchor line (K = 2)
  c_empty     all slots empty (K = 2): the cost of the call itself over mw_ocean_step_fleet

mw_ocean_step_rigged always steps per substep; mw_ocean_step_fleet takes its own plan (the buoys in one launch on the periodic handle).
Every timed call starts from the same state (a device copy before the call, timed with it).

Usage: python tools/rig_bench.py [--reps 50]"""
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
from fleet_bench import scenes, timed_alternating  # noqa: E402

CHAIN = 8


def anchor_lines(lines, slot, bodies, mass, rng, who):
    """one taut anchor line in `slot` of the bodies `who`: the anchor 8 to 12 away, below and around (moorings_bench.lines_for)"""
    n = len(who)
    u = rng.standard_normal((n, 3))
    u[:, 1] = -1.0 - np.abs(u[:, 1])
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    dist = rng.uniform(8.0, 12.0, n)
    lines[who, slot, 0:3] = rng.uniform(-0.5, 0.5, (n, 3))
    lines[who, slot, 4:7] = bodies[who, 0:3] + u * dist[:, None]
    lines[who, slot, 3], lines[who, slot, 7], lines[who, slot, 8] = 0.8 * dist, 2.0 * mass[who, 0], 0.5 * mass[who, 0]


def configurations(bodies, mass, counts, rng):
    """(name, lines [n, K, 12], targets [n, K]) of the three configurations; counts = bodies per hull (buoys, barges, the big hull)"""
    n = len(bodies)
    everyone = np.arange(n)
    lines, targets = mw.pack_lines(n, 1), np.full((n, 1), mw.MW_RIG_ANCHOR, np.int32)
    anchor_lines(lines, 0, bodies, mass, rng, everyone)
    yield "a_anchored", lines, targets
    lines, targets = mw.pack_lines(n, 2), np.full((n, 2), mw.MW_RIG_ANCHOR, np.int32)
    first = counts[0]
    barges = np.arange(first, first + counts[1])
    anchor_lines(lines, 0, bodies, mass, rng, np.setdiff1d(everyone, barges))
    fore, aft = np.array([0.0, 0.5, 9.0], np.float32), np.array([0.0, 0.5, -9.0], np.float32)
    for b in barges:
        if (b - first) % CHAIN == 0:
            continue  # the first of a chain tows and is not towed
        gap = float(np.linalg.norm(bodies[b, 0:3] - bodies[b - 1, 0:3]))
        # slot 0 of b (fore) to slot 1 of b - 1 (aft), mirrored; 10 % stretched
        for own, slot, h, other, a in ((b, 0, fore, b - 1, aft), (b - 1, 1, aft, b, fore)):
            lines[own, slot, 0:3], lines[own, slot, 4:7] = h, a
            lines[own, slot, 3], lines[own, slot, 7], lines[own, slot, 8] = 0.9 * gap, 2.0 * mass[b, 0], 0.5 * mass[b, 0]
            targets[own, slot] = other
    yield "b_towed", lines, targets
    yield "c_empty", mw.pack_lines(n, 2), np.full((n, 2), mw.MW_RIG_ANCHOR, np.int32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--substeps", type=int, default=8)
    a = ap.parse_args()
    if a.reps < 30:
        ap.error("--reps must be at least 30")
    nat.require_product_build("rig_bench")
    stream = torch.cuda.current_stream()
    p = workloads.fftmesh_params(1024)
    o = mw.Ocean(resolution=1024, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                 choppiness=p.choppiness, gravity=p.gravity, device=0)
    o.set_stream(stream.cuda_stream)
    o.evaluate(2.0)
    K, dt = a.substeps, 1.0 / 60
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()  # noqa: E731
    name, scene = next(scenes())
    assert name == "a_scene"
    hulls, masses, allb = [], [], []
    for (hull0, tris), b in scene:
        m, c, I = mw.hull_mass_properties(hull0, tris, 500.0)
        hulls.append((np.ascontiguousarray(hull0 - c, np.float32), tris, len(b)))
        masses.append(mw.pack_mass(np.full(len(b), m), np.broadcast_to(I, (len(b), 3, 3))))
        allb.append(b)
    x, t, table = mw.pack_fleet(hulls)
    bodies, mass = np.concatenate(allb), np.concatenate(masses)
    n = len(bodies)
    d_x, d_t, d_b0, d_m = up(x), up(t), up(bodies), up(mass)
    d_b, d_o = d_b0.clone(), torch.empty((n, 8), device="cuda")
    cf = [1000.0, 9.81, 0.0, 0.0, np.nan]
    rng = np.random.default_rng(2)
    rows = []
    for cname, lines, targets in configurations(bodies, mass, [len(b) for b in allb], rng):
        nl = lines.shape[1]
        d_l, d_g, d_n = up(lines), up(targets), torch.empty((n, nl), device="cuda")
        torch.cuda.synchronize()
        for periodic in (True, False):
            o.set_periodic(periodic)

            def fleet_step():
                d_b.copy_(d_b0)
                o.step_fleet_device(d_x.data_ptr(), len(x), d_t.data_ptr(), len(t), table, d_b.data_ptr(), d_m.data_ptr(), n, dt, K,
                                    d_out=d_o.data_ptr(), coeffs=cf)

            def rigged_step():
                d_b.copy_(d_b0)
                o.step_rigged_device(d_x.data_ptr(), len(x), d_t.data_ptr(), len(t), table, d_b.data_ptr(), d_m.data_ptr(), d_l.data_ptr(), nl, n,
                                     dt, K, d_targets=d_g.data_ptr(), d_out=d_o.data_ptr(), d_tension=d_n.data_ptr(), coeffs=cf)
            t_us = timed_alternating(stream, a.reps, {"step_fleet": fleet_step, "step_rigged": rigged_step})
            rigged_step()
            torch.cuda.synchronize()
            ten = d_n.cpu().numpy()
            rows.append(dict(t_us, case=cname, periodic=periodic, total_bodies=n, total_verts=len(x), total_tris=len(t), substeps=K,
                             lines_per_body=nl, tow_slots=int((targets >= 0).sum()), taut_lines=int((ten > 0).sum()),
                             finite_rows=int(np.isfinite(d_o.cpu().numpy()).all(1).sum()),
                             ratio=t_us["step_rigged"]["median"] / t_us["step_fleet"]["median"],
                             over_step_fleet_us=t_us["step_rigged"]["median"] - t_us["step_fleet"]["median"]))
    o.set_periodic(False)
    o.set_stream(None)
    o.close()
    line = json.dumps({"tool": "rig_bench", "build": nat.build_id(), "device": torch.cuda.get_device_name(0), "reps": a.reps, "rows": rows})
    print(line)
    path = os.path.join(REPO, "profiles", "rig_bench_%s.json" % nat.build_id().split(" ")[0])
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
