"""The water column (mw_ocean_set_column / mw_ocean_query_column) on the 1024^2 FFTMesh: what the layers cost to build and what a query
costs by how deep it has to scan.  HIP events on the handle's stream (torch's current stream), median of --reps.  Prints one JSON line
and writes it to profiles/column_bench_<build id>.json.  Geometric depths 2, 4, 8, ... with L = 4 and L = 8 layers.

  build    the layer arrays after a new frame (spectrum unchanged: frame passes only), and the first build after a spectrum change
           (the weight kernel and the prep tables of every layer on top); the frame itself is made outside the timed region
  world    10^6 points with y uniform between the surface and the deepest layer; the same points all within the top interval; the same
           points all below the deepest layer
  rest     10^6 labels with d uniform in [0, d_{L-1}]
  periodic the first world case spread over 7 x 7 tiles, on a periodic handle

usage: python tools/column_bench.py [--reps R]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    a = ap.parse_args()
    nat.require_product_build("column_bench")
    stream = torch.cuda.current_stream()
    p = workloads.fftmesh_params(1024)
    o = mw.Ocean(resolution=1024, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                 choppiness=p.choppiness, gravity=p.gravity, device=0)
    o.set_stream(stream.cuda_stream)
    vert = o.evaluate(2.0)[0]
    h0, h0c = o.get_spectrum()
    P, uw = o.period, p.unit_width
    x0 = (0 - 512) * uw + uw / 2
    rest = x0 + uw * np.arange(1024)
    dmax = float(np.abs(vert[:, [0, 2]] - np.stack(np.meshgrid(rest, rest, indexing="ij"), -1).reshape(-1, 2)).max())
    n = 1000000
    rng = np.random.default_rng(n)
    inside = rng.uniform(rest[0] + dmax, rest[-1] - dmax, (n, 2)).astype(np.float32)
    spread = rng.uniform(x0 - 3 * P, x0 + 4 * P, (n, 2)).astype(np.float32)
    frac = rng.random(n)
    d_out = torch.empty((n, 12), device="cuda")
    rows = []
    tick = [2.0]

    def new_frame():
        tick[0] += 0.125
        o.evaluate(tick[0])

    def new_spectrum():
        o.set_spectrum(h0, h0c)
        new_frame()

    for L in (4, 8):
        depths = np.concatenate([[0.0], 2.0 * 2.0 ** np.arange(L - 1)]).astype(np.float32)
        deep = float(depths[-1])
        o.set_periodic(False)
        o.set_column(depths)
        rows.append({"case": "build", "layers": L, "after_frame_us": timed(stream, a.reps, lambda: o.column_layers(1), before=new_frame),
                     "after_spectrum_us": timed(stream, a.reps, lambda: o.column_layers(1), before=new_spectrum)})

        def query_row(case, xyz, mode, periodic=False):
            o.set_periodic(periodic)
            q = np.zeros((n, 4), np.float32)
            q[:, :3] = xyz
            d_q = torch.from_numpy(q).cuda()
            o.column_layers(1)
            torch.cuda.synchronize()
            t = timed(stream, a.reps, lambda: o.query_column_device(d_q.data_ptr(), n, d_out.data_ptr(), mode=mode))
            out = d_out.cpu().numpy()
            lam = out[:, 7]
            rows.append({"case": case, "layers": L, "mode": mode, "periodic": periodic, "n": n, "query_us": t,
                         "mean_lambda": float(np.nanmean(lam)), "nan_rows": int(np.isnan(lam).sum()),
                         "resolved_fraction": float(np.mean(out[:, 11] <= 1e-4 * uw))})

        eta = o.query_surface(inside, mode="world")[:, 1]
        col = lambda y: np.stack([inside[:, 0], y, inside[:, 1]], 1)
        query_row("world_uniform", col(eta - frac * deep), "world")
        query_row("world_top_interval", col(eta - frac * 0.5 * float(depths[1])), "world")
        query_row("world_below_deepest", col(-deep - 10.0 - 10.0 * frac), "world")
        query_row("rest_uniform", col(frac * deep), "rest")
        o.set_periodic(True)
        eta_t = o.query_surface(spread, mode="world")[:, 1]
        query_row("world_uniform_7x7_tiles", np.stack([spread[:, 0], eta_t - frac * deep, spread[:, 1]], 1), "world", periodic=True)
    o.set_periodic(False)
    o.set_stream(None)
    o.close()
    line = json.dumps({"tool": "column_bench", "build": nat.build_id(), "device": torch.cuda.get_device_name(0), "rows": rows})
    print(line)
    path = os.path.join(REPO, "profiles", "column_bench_%s.json" % nat.build_id().split(" ")[0])
    with open(path, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
