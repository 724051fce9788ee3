"""Occlusion rays generated on the device, measured: what a whole ambient-occlusion call costs when no ray crosses the bus, and
what building a ray in registers costs next to reading it from HBM.

    python scripts/gpu_occlusion.py [--out DIR]

One child process per scene, each under its own time limit; the first failure ends the run.  Every child writes DIR/occlusion_<scene>.json.  The view
is 1920 x 1080 with 8 directions (4 targets) per first hit; a warm-up, then the median of 5, the compared calls alternated in one process:

  (a) whole call   wall time (a host clock around calls that end synchronised, host arrays in and out) of DeviceScene.ambient_occlusion -- first hits
                   downloaded, camera.hemisphere_rays in numpy, the rays uploaded -- against DeviceScene.ambient_occlusion_device's host form
  (b) hemisphere   device time (RTMI_FLAG_TIMING: the query kernel alone) of rtmi_occlusion_hemisphere_device, counts only, against
                   rtmi_query_occluded_device on the same rays resident in HBM -- the call's own out_rays, so both trace identical rays
  (c) targets      the same for rtmi_occlusion_targets_device with 4 targets

  scenes: C3 = the cover scene with 10 001 spheres; cornell = the Cornell box
The child fails (exit status 1) if the generated-source counts are not the memory-source counts."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIMIT = 420  # seconds per scene
REPS = 5
VIEW = (1920, 1080)
N_DIRS = 8
N_TARGETS = 4
RADIUS = 1.0
SCENES = ("C3", "cornell")
TARGETS = {"C3": [[0.0, 40.0, 0.0], [13.0, 2.0, 3.0], [-20.0, 15.0, 5.0], [5.0, 30.0, -25.0]],
           "cornell": [[278.0, 554.0, 279.5], [213.0, 554.0, 227.0], [343.0, 554.0, 332.0], [278.0, 278.0, -800.0]]}


def _median(samples):
    return {"median_ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples), "n": len(samples)}


def measure(which):
    import numpy as np
    import torch

    import raytrace_clj_amd as r
    from raytrace_clj_amd import _ffi, core
    nx, ny = VIEW
    sc = r.scene.make_random_scene(nx, ny, 50, False) if which == "C3" else r.scene.make_cornell_box(nx, ny)
    ctx = core.Context(0, timing=True)
    ds = core.DeviceScene(sc, ctx=ctx)
    n = nx * ny
    res = {"scene": which, "view": list(VIEW), "points": n, "n_dirs": N_DIRS, "n_targets": N_TARGETS, "primitives": int(len(ds.flat.prim_kind))}

    # (a) the whole call, host arrays in and out
    t_old, t_new = [], []
    for rep in range(REPS + 1):  # the two alternate; repetition 0 warms up (workspace, occupancy queries, staging arena)
        t0 = time.perf_counter()
        old = ds.ambient_occlusion(nx, ny, N_DIRS, RADIUS)
        t1 = time.perf_counter()
        new = ds.ambient_occlusion_device(nx, ny, N_DIRS, RADIUS)
        t2 = time.perf_counter()
        if rep:
            t_old.append((t1 - t0) * 1e3), t_new.append((t2 - t1) * 1e3)
    res["whole_call_ambient_occlusion"], res["whole_call_ambient_occlusion_device"] = _median(t_old), _median(t_new)
    res["whole_call_new_over_old"] = statistics.median(t_new) / statistics.median(t_old)
    res["image_means"] = [float(old.mean()), float(new.mean())]
    res["uploaded_ray_bytes_old_path"] = n * N_DIRS * 7 * 8
    del old, new

    # the points: the first hits of the pixel-centre rays, resident
    primary = ds.pixel_centre_rays(nx, ny)
    d_view = torch.from_numpy(primary).cuda()
    d_hits = torch.zeros((n, _ffi.HIT_REC), dtype=torch.float64, device="cuda")
    d_count = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_count2 = torch.zeros(n, dtype=torch.int32, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ds.query_hits_device(n, d_view, d_hits)
    torch.cuda.synchronize()
    res["points_hit"] = int((d_hits[:, 0] != 0).sum().item())
    d_tg = torch.tensor(TARGETS[which], dtype=torch.float64, device="cuda")

    def compare(tag, per, generated, t_min, t_max):
        d_rays = torch.zeros((n * per, 7), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        generated(d_rays, d_count2)  # the rays both sides trace
        torch.cuda.synchronize()
        t_gen, t_mem = [], []
        for rep in range(REPS + 1):
            generated(None, d_count)
            a = ctx.last_trace_ms()[0]
            ds.occluded_device(n, per, d_rays, out_count=d_count2, t_min=t_min, t_max=t_max)
            b = ctx.last_trace_ms()[0]
            if rep:
                t_gen.append(a), t_mem.append(b)
        torch.cuda.synchronize()
        res[tag] = {"generated_source": _median(t_gen), "memory_source": _median(t_mem), "rays": n * per, "rays_generated": int(cnt.cpu().numpy()[0]),
                    "occluded": int(d_count.sum().item()), "counts_are_the_memory_sources": bool(torch.equal(d_count, d_count2)),
                    "generated_over_memory": statistics.median(t_gen) / statistics.median(t_mem)}
        del d_rays

    # (b) 8 hemisphere rays per first hit, (c) 4 targets
    compare("hemisphere", N_DIRS, lambda d_rays, d_c: ds.occlusion_hemisphere_device(n, d_hits, N_DIRS, view=d_view, seed=core.RENDER_SEED, t_min=0.001,
                                                                                        t_max=RADIUS, out_count=d_c, out_rays=d_rays, out_counters=cnt),
            0.001, RADIUS)
    compare("targets", N_TARGETS, lambda d_rays, d_c: ds.occlusion_targets_device(n, d_hits, N_TARGETS, d_tg, view=d_view, t_min=0.001, t_max=1.0 - 0.001,
                                                                                   out_count=d_c, out_rays=d_rays, out_counters=cnt),
            0.001, 1.0 - 0.001)
    ds.close()
    ctx.close()
    res["ok"] = all(res[tag]["counts_are_the_memory_sources"] for tag in ("hemisphere", "targets"))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "occlusion"))
    ap.add_argument("--child", default=None, choices=SCENES)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        res = measure(a.child)
        with open(os.path.join(a.out, "occlusion_%s.json" % a.child), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res), flush=True)
        if not res["ok"]:
            print("the generated source's counts are not the memory source's: the timings compare different work", flush=True)
            return 1
        return 0
    for which in SCENES:
        print("== occlusion, scene %s (limit %d s)" % (which, LIMIT), flush=True)
        try:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--out", a.out], check=True, timeout=LIMIT, cwd=ROOT)
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
            print("the measurement failed: %s" % e, flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
