"""Path tracing with next-event estimation, measured: what the second traversal costs per path, and what the light samples buy
in error.

    python scripts/gpu_nee.py [--out DIR] [--only paths|error]

One child process per measurement, each under its own time limit; the first failure ends the run.  Every child writes DIR/nee_<name>.json.  A warm-up,
then the median of 5 with minimum - maximum, the compared calls alternated in one process:

  paths  device time (RTMI_FLAG_TIMING: the path kernel alone) of rtmi_render_rays_nee_device against rtmi_render_rays_device on the same
         1920 x 1080 x 4 pinhole rays (the pixel-centre rays, four paths each, keys derived), depth 50, per scene:
         C3 = the cover scene with 10 001 spheres and one added sphere lamp; cornell = the Cornell box.  Reported per path, with the counters.
  error  the Cornell box at 256 x 256: RMS error (over pixels and channels, linear radiance) against a 4 096-spp frame of rtmi_render, of the plain
         and the light-sampled estimator over the same camera rays (DeviceScene.render_nee, the plain one with an empty light list) at equal
         samples, and of the plain one at the samples the light-sampled frame's device time pays for (equal time).  Beside the RMS error: the
         median over pixels of the absolute error, and the share of the squared error held by the worst 0.1 % of the pixels -- one light sample per
         vertex has a heavy tail next to a lamp (the inverse square of area sampling), and a few pixels can carry the RMS figure."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIMIT = 540  # seconds per child
REPS = 5
VIEW = (1920, 1080)
PER_PIXEL = 4
DEPTH = 50
FRAME, REFERENCE_SPP, SPP = 256, 4096, 16
CHILDREN = ("paths_C3", "paths_cornell", "error")


def _median(samples):
    return {"median_ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples), "n": len(samples)}


def _scene(which, nx, ny):
    import raytrace_clj_amd as r
    from raytrace_clj_amd import hitable as hit
    from raytrace_clj_amd import shader as shad
    from raytrace_clj_amd import texture as tex
    from raytrace_clj_amd.util import vec3
    if which == "cornell":
        return r.scene.make_cornell_box(nx, ny)
    sc = r.scene.make_random_scene(nx, ny, 50, False, bvh=False)
    lamp = hit.sphere(center=vec3(0, 12, 0), radius=3, material=shad.diffuse_light(tex=tex.constant(color=vec3(8, 8, 8))))
    return {"camera": sc["camera"], "world": hit.hitlist(items=list(sc["world"].items) + [lamp])}


def measure_paths(which):
    import numpy as np
    import torch

    from raytrace_clj_amd import core
    nx, ny = VIEW
    ctx = core.Context(0, timing=True)
    ds = core.DeviceScene(_scene(which, nx, ny), ctx=ctx)
    ng, n = nx * ny, nx * ny * PER_PIXEL
    d_rays = torch.from_numpy(np.repeat(ds.pixel_centre_rays(nx, ny), PER_PIXEL, axis=0)).cuda()
    mean = [torch.zeros((ng, 3), dtype=torch.float64, device="cuda") for _ in range(2)]
    err = torch.zeros(ng, dtype=torch.float64, device="cuda")
    cnt = [torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros(4, dtype=torch.int64, device="cuda")]
    t_plain, t_nee = [], []
    for rep in range(REPS + 1):
        ds.render_rays_device(ng, PER_PIXEL, d_rays, mean[0], err, depth=DEPTH, out_counters=cnt[0])
        a = ctx.last_trace_ms()[0]
        ds.render_rays_nee_device(ng, PER_PIXEL, d_rays, mean[1], err, depth=DEPTH, out_counters=cnt[1])
        b = ctx.last_trace_ms()[0]
        if rep:
            t_plain.append(a), t_nee.append(b)
        print("rep %d: plain %.2f ms, light-sampled %.2f ms" % (rep, a, b), flush=True)
    torch.cuda.synchronize()
    plain, nee = (c.cpu().numpy().tolist() for c in cnt)
    res = {"scene": which, "view": list(VIEW), "paths": n, "depth": DEPTH, "primitives": int(len(ds.flat.prim_kind)), "lights": ds.lights().tolist(),
           "library": os.path.basename(core._ffi.LIB_PATH),
           "plain": _median(t_plain), "light_sampled": _median(t_nee), "light_sampled_over_plain": statistics.median(t_nee) / statistics.median(t_plain),
           "plain_ns_per_path": statistics.median(t_plain) * 1e6 / n, "light_sampled_ns_per_path": statistics.median(t_nee) * 1e6 / n,
           "segments": nee[0], "shadow_rays_built": nee[2], "shadow_rays_occluded": nee[3],
           "mean_plain": float(mean[0].mean().item()), "mean_light_sampled": float(mean[1].mean().item())}
    res["ok"] = plain[0] == nee[0] and plain[1] == nee[1] == n  # the same paths: the same segments
    ds.close()
    ctx.close()
    return res


def measure_error():
    import numpy as np

    from raytrace_clj_amd import core
    ctx = core.Context(0, timing=True)
    ds = core.DeviceScene(_scene("cornell", FRAME, FRAME), ctx=ctx)
    reference = ds.render(FRAME, FRAME, REFERENCE_SPP, seed=0xBEEF)[0]
    ctx.last_trace_ms()
    print("reference: %d spp, mean %.4f" % (REFERENCE_SPP, reference.mean()), flush=True)

    def rms(frame):
        return float(np.sqrt(np.mean((frame - reference) ** 2)))

    def mae(frame):  # the median over pixels of the absolute error of the channel sum: what most of the frame looks like, whatever a few outliers do
        return float(np.median(np.abs((frame - reference).sum(axis=2))))

    def worst(frame):  # the share of the squared error that the worst 0.1 % of the pixels hold
        e = np.sort(((frame - reference) ** 2).sum(axis=2).ravel())
        return float(e[-max(1, len(e) // 1000):].sum() / e.sum())

    def frame(ns, lights, seed):
        lin = ds.render_nee(FRAME, FRAME, ns, min(ns, 16), seed=seed, lights=lights)[0]
        return lin, ctx.last_trace_ms()[0]
    frame(SPP, None, 1), frame(SPP, [], 1)  # warm-up
    rows = []
    for rep in range(REPS):
        nee, t_nee = frame(SPP, None, 100 + rep)
        plain, t_plain = frame(SPP, [], 100 + rep)
        more = max(SPP, int(round(SPP * t_nee / t_plain)))
        longer, t_longer = frame(more, [], 100 + rep)
        rows.append({"rms_light_sampled": rms(nee), "rms_plain_equal_samples": rms(plain), "rms_plain_equal_time": rms(longer),
                     "median_abs_light_sampled": mae(nee), "median_abs_plain_equal_samples": mae(plain), "median_abs_plain_equal_time": mae(longer),
                     "worst_permille_share_light_sampled": worst(nee), "worst_permille_share_plain_equal_samples": worst(plain), "ms_light_sampled": t_nee,
                     "ms_plain_equal_samples": t_plain, "plain_spp_equal_time": more, "ms_plain_equal_time": t_longer})
        print(json.dumps(rows[-1]), flush=True)
    res = {"scene": "cornell", "frame": [FRAME, FRAME], "reference_spp": REFERENCE_SPP, "spp": SPP, "reps": rows, "mean_reference": float(reference.mean())}
    for key in rows[0]:
        vals = [r[key] for r in rows]
        res[key] = {"median": statistics.median(vals), "min": min(vals), "max": max(vals)}
    res["error_ratio_equal_samples"] = res["rms_plain_equal_samples"]["median"] / res["rms_light_sampled"]["median"]
    res["error_ratio_equal_time"] = res["rms_plain_equal_time"]["median"] / res["rms_light_sampled"]["median"]
    res["ok"] = True
    ds.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "nee"))
    ap.add_argument("--only", default=None, choices=("paths", "error"))
    ap.add_argument("--child", default=None, choices=CHILDREN)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        res = measure_error() if a.child == "error" else measure_paths(a.child.split("_", 1)[1])
        with open(os.path.join(a.out, "nee_%s.json" % a.child), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({k: v for k, v in res.items() if k != "reps"}), flush=True)
        if not res["ok"]:
            print("the light-sampled call did not trace the plain call's paths: the timings compare different work", flush=True)
            return 1
        return 0
    for which in CHILDREN:
        if a.only and not which.startswith(a.only):
            continue
        print("== light-sampled paths, %s (limit %d s)" % (which, LIMIT), flush=True)
        try:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--out", a.out], check=True, timeout=LIMIT, cwd=ROOT)
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
            print("the measurement failed: %s" % e, flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
