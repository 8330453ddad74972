"""Surface queries (mw_ocean_query_surface / _device): time per call for n = 10^3 and 10^6 points, rest and world mode, FFTMesh 1024^2
and OceanRenderer resolution 128 (1024^2 textures), host and device forms, against a numpy restatement of the same query on the CPU.
Device form: HIP events around back-to-back calls on the handle's stream (torch's current stream); host form: wall clock of the
synchronous call (PCIe both ways included).  Prints one JSON line.
usage: python tools/query_bench.py [--reps R] [--iterations K] [--no-numpy]"""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "mistral-water_amd"), os.path.join(REPO, "tests")]
import torch  # noqa: E402  (initialises its HIP runtime before the library)
torch.cuda.init()
import numpy as np  # noqa: E402
import mistral_water as mw  # noqa: E402
from mistral_water import _native as nat  # noqa: E402
import workloads  # noqa: E402


def rest_coords(R, uw):
    base = (np.arange(R) - R // 2).astype(np.float32) * np.float32(uw)
    return (base + np.float32(uw) / np.float32(2)).astype(np.float32) if R % 2 == 0 else base


def numpy_query(vert, norm, white, R, uw, xz, world, iters):
    """numpy restatement of csrc/surface_query.h (vectorised over the points; float32 like the kernel): the CPU baseline."""
    rc = rest_coords(R, uw)
    lo, hi = rc[0], rc[-1]
    qx, qz = xz[:, 0], xz[:, 1]

    def cell(x):
        i = np.clip(np.floor((x - lo) / np.float32(uw)), 0, R - 2).astype(np.int64)
        return i, (x - rc[i]) / (rc[i + 1] - rc[i])

    def tri(i, j, fa, fb):
        up = fa + fb > 1
        c = i * R + j
        v = np.where(up[:, None], np.stack([c + R + 1, c + R, c + 1], -1), np.stack([c, c + R, c + 1], -1))
        w = np.where(up[:, None], np.stack([fa + fb - 1, 1 - fb, 1 - fa], -1), np.stack([1 - fa - fb, fa, fb], -1))
        return up, v, w.astype(np.float32)

    ux, uz = np.clip(qx, lo, hi), np.clip(qz, lo, hi)
    i, fa = cell(ux)
    j, fb = cell(uz)
    if world:
        done = np.zeros(len(xz), bool)
        bi, bj, bfa, bfb, best = i.copy(), j.copy(), fa.copy(), fb.copy(), np.full(len(xz), np.inf, np.float32)
        for it in range(iters + 1):
            up, v, w = tri(i, j, fa, fb)
            px, pz = vert[v, 0], vert[v, 2]
            o_x = np.where(up, px[:, 1] + px[:, 2] - px[:, 0], px[:, 0])
            o_z = np.where(up, pz[:, 1] + pz[:, 2] - pz[:, 0], pz[:, 0])
            ax = np.where(up, px[:, 0] - px[:, 2], px[:, 1] - px[:, 0])
            az = np.where(up, pz[:, 0] - pz[:, 2], pz[:, 1] - pz[:, 0])
            bx = np.where(up, px[:, 0] - px[:, 1], px[:, 2] - px[:, 0])
            bz = np.where(up, pz[:, 0] - pz[:, 1], pz[:, 2] - pz[:, 0])
            det = ax * bz - bx * az
            with np.errstate(divide="ignore", invalid="ignore"):
                sa = ((qx - o_x) * bz - bx * (qz - o_z)) / det
                sb = (ax * (qz - o_z) - (qx - o_x) * az) / det
            t = np.float32(1e-5)
            inside = np.where(up, (sa <= 1 + t) & (sb <= 1 + t) & (sa + sb >= 1 - t), (sa >= -t) & (sb >= -t) & (sa + sb <= 1 + t))
            hit = inside & ~done
            bi[hit], bj[hit] = i[hit], j[hit]
            bfa[hit], bfb[hit] = np.clip(sa[hit], 0, 1), np.clip(sb[hit], 0, 1)
            done |= hit
            ex, ez = (w * px).sum(1) - qx, (w * pz).sum(1) - qz
            r = ex * ex + ez * ez
            better = ~done & (r < best)
            best[better], bi[better], bj[better], bfa[better], bfb[better] = r[better], i[better], j[better], fa[better], fb[better]
            if it == iters or done.all():
                break
            da, db = sa - fa, sb - fb
            ln = np.maximum(np.abs(da), np.abs(db))
            newton = (det > 0) & (ln <= 1e30)
            k = np.where(ln > 4, 4 / np.where(ln > 0, ln, 1), 1).astype(np.float32)
            ux = np.where(newton, ux + da * k * np.float32(uw), ux - ex)
            uz = np.where(newton, uz + db * k * np.float32(uw), uz - ez)
            ux, uz = np.clip(ux, lo, hi), np.clip(uz, lo, hi)
            i, fa = cell(ux)
            j, fb = cell(uz)
        i, j, fa, fb = bi, bj, bfa, bfb
    _, v, w = tri(i, j, fa, fb)
    p = (w[..., None] * vert[v]).sum(1)
    n = (w[..., None] * norm[v]).sum(1)
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    out = np.concatenate([p, n, (w * white[v]).sum(1)[:, None], np.hypot(p[:, 0] - qx, p[:, 2] - qz)[:, None] if world
                          else np.zeros((len(xz), 1), np.float32)], 1)
    if not world:
        out[(qx < lo) | (qx > hi) | (qz < lo) | (qz > hi)] = np.nan
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--iterations", type=int, default=0, help="0 = the library default (8)")
    ap.add_argument("--no-numpy", action="store_true")
    a = ap.parse_args()
    nat.require_product_build("query_bench")
    stream = torch.cuda.current_stream()
    rows = []
    p = workloads.fftmesh_params(1024)
    oceans = {
        "fftmesh_1024": mw.Ocean(resolution=1024, unit_width=p.unit_width, length=p.length, wind=(p.wind_x, p.wind_y), amplitude=p.amplitude,
                                 choppiness=p.choppiness, gravity=p.gravity, device=0),
        "oceanrenderer_128": mw.Ocean(resolution=128, length=434.48, wind=(14.45, 12.0), amplitude=0.41, choppiness=1.5, mult=1.5,
                                      semantics=nat.MW_SEM_OCEANRENDERER, device=0),
    }
    for name, o in oceans.items():
        o.set_stream(stream.cuda_stream)
        if o.semantics == nat.MW_SEM_FFTMESH:
            vert, norm, col = o.evaluate(2.0)
            white, R, uw = col[:, 0].copy(), 1024, p.unit_width
        else:
            o.generate_texture(1.0 / 60.0)
            vert, norm, white = o.displace_mesh()
            R, uw = 128, 1.0
        rc = rest_coords(R, uw)
        dmax = float(np.abs(vert[:, [0, 2]] - np.stack(np.meshgrid(rc, rc, indexing="ij"), -1).reshape(-1, 2)).max())
        for n in (1000, 1000000):
            xz = np.random.default_rng(n).uniform(rc[0] + dmax, rc[-1] - dmax, (n, 2)).astype(np.float32)
            d_xz = torch.from_numpy(xz).cuda()
            d_out = torch.empty((n, 8), device="cuda")
            for mode in ("rest", "world"):
                row = {"workload": name, "n": n, "mode": mode}
                # device form: HIP events around reps back-to-back calls
                for _ in range(3):
                    o.query_surface_device(d_xz.data_ptr(), n, d_out.data_ptr(), mode=mode, iterations=a.iterations)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
                per = []
                for _ in range(a.reps):
                    ev[0].record(stream)
                    o.query_surface_device(d_xz.data_ptr(), n, d_out.data_ptr(), mode=mode, iterations=a.iterations)
                    ev[1].record(stream)
                    ev[1].synchronize()
                    per.append(ev[0].elapsed_time(ev[1]) * 1e3)
                row["device_us_median"] = float(np.median(per))
                row["device_us_min"] = float(np.min(per))
                dev = d_out.cpu().numpy()
                # host form: wall clock of the synchronous call
                host = o.query_surface(xz, mode=mode, iterations=a.iterations)
                per = []
                for _ in range(max(3, a.reps // 4)):
                    t0 = time.perf_counter()
                    o.query_surface(xz, mode=mode, iterations=a.iterations)
                    per.append((time.perf_counter() - t0) * 1e6)
                row["host_us_median"] = float(np.median(per))
                row["host_equals_device"] = bool(np.array_equal(host.view(np.uint32), dev.view(np.uint32)))
                if mode == "world":
                    row["resolved_fraction"] = float(np.mean(host[:, 7] <= 1e-4 * uw))
                if not a.no_numpy:
                    t0 = time.perf_counter()
                    ref = numpy_query(vert, norm, white, R, uw, xz, mode == "world", a.iterations or 8)
                    row["numpy_us"] = (time.perf_counter() - t0) * 1e6
                    row["numpy_max_dy"] = float(np.nanmax(np.abs(ref[:, 1] - host[:, 1])))
                rows.append(row)
        o.set_stream(None)
        o.close()
    print(json.dumps({"tool": "query_bench", "build": nat.build_id(), "device": torch.cuda.get_device_name(0),
                      "iterations": a.iterations or 8, "rows": rows}))


if __name__ == "__main__":
    main()
