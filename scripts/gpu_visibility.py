"""Closest-hit and any-hit queries on the GPU, measured: what rtmi_query_hits_device costs next to the path kernel asked for the
same first hits, and what leaving at the first accepted primitive (rtmi_query_occluded_device) is worth next to the closest-hit search on the same
secondary rays.

    python scripts/gpu_visibility.py [--out DIR]

One child process per scene, each under its own time limit; the first failure ends the run.  Every child writes DIR/visibility_<scene>.json.  The view
is 1920 x 1080; a warm-up, then the median of 5, the compared calls alternated in one process, by the library's own events (RTMI_FLAG_TIMING: the
trace interval, i.e. the query kernel or rays_kernel alone):

  (a) primary    the pixel-centre rays: rtmi_query_hits_device against rtmi_render_rays_device with depth 0 on the same rays
  (b) secondary  8 camera.hemisphere_rays per first hit, t-range (0.001, 1.0) and (0.001, Float/MAX_VALUE): rtmi_query_occluded_device (group 8, counts
                 only) against rtmi_query_hits_device on the same rays
  (c) counters   the sums of rtmi_last_traversal_counters (AABB + primitive tests) of the four calls of (b), option count_traversal = 1 (C3 only: the
                 counting instantiation exists for the FP64 sphere tree)

  scenes: C3 = the cover scene with 10 001 spheres; cornell = the Cornell box (18 rectangles; option flat_below sends it to the small-world scan)
The child also states whether the any-hit flags are the closest-hit search's."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIMIT = 420  # seconds per scene
REPS = 5
VIEW = (1920, 1080)
N_DIRS = 8
SCENES = ("C3", "cornell")
FLT_MAX = 3.4028234663852886e38


def _median(samples):
    return {"median_ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples), "n": len(samples)}


def measure(which):
    import numpy as np
    import torch

    import raytrace_clj_amd as r
    from raytrace_clj_amd import _ffi, core
    from raytrace_clj_amd import camera as cam
    nx, ny = VIEW
    sc = r.scene.make_random_scene(nx, ny, 50, False) if which == "C3" else r.scene.make_cornell_box(nx, ny)
    ctx = core.Context(0, timing=True)
    ds = core.DeviceScene(sc, ctx=ctx)
    n = nx * ny
    res = {"scene": which, "view": list(VIEW), "primary_rays": n, "primitives": int(len(ds.flat.prim_kind)), "tree_info": list(ds.tree_info())}

    # (a) the pixel-centre rays
    primary = ds.pixel_centre_rays(nx, ny)
    d_rays = torch.from_numpy(primary).cuda()
    d_hits = torch.zeros((n, _ffi.HIT_REC), dtype=torch.float64, device="cuda")
    mean = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    err = torch.zeros(n, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    t_query, t_paths = [], []
    for rep in range(REPS + 1):  # the two alternate; repetition 0 warms up (workspace, occupancy queries)
        ds.query_hits_device(n, d_rays, d_hits, out_counters=cnt)
        a = ctx.last_trace_ms()[0]
        ds.render_rays_device(n, 1, d_rays, mean, err, depth=0, ctr0=2)
        b = ctx.last_trace_ms()[0]
        if rep:
            t_query.append(a), t_paths.append(b)
    torch.cuda.synchronize()
    res["primary_query_hits"], res["primary_render_rays_depth0"] = _median(t_query), _median(t_paths)
    res["primary_counters"] = [int(x) for x in cnt.cpu().numpy()]
    hits = d_hits.cpu().numpy()
    del d_hits, mean, err, d_rays

    # (b) 8 hemisphere rays per first hit
    hit = hits[:, 0] != 0.0
    normals = hits[hit, 6:9].copy()
    away = (normals * primary[hit, 3:6]).sum(axis=1) > 0.0
    normals[away] = -normals[away]
    sec = cam.hemisphere_rays(hits[hit, 3:6], normals, N_DIRS, seed=core.RENDER_SEED, time=float(primary[0, 6]))
    groups, m = int(hit.sum()), int(hit.sum()) * N_DIRS
    res["secondary_rays"] = m
    d_sec = torch.from_numpy(sec).cuda()
    del sec, hits, normals
    d_rec = torch.zeros((m, _ffi.HIT_REC), dtype=torch.float64, device="cuda")
    d_flags = torch.zeros(m, dtype=torch.uint8, device="cuda")
    d_count = torch.zeros(groups, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    for tag, t_max in (("radius_1", 1.0), ("unbounded", FLT_MAX)):
        t_any, t_closest = [], []
        for rep in range(REPS + 1):
            ds.occluded_device(groups, N_DIRS, d_sec, out_count=d_count, t_max=t_max, out_counters=cnt)
            a = ctx.last_trace_ms()[0]
            ds.query_hits_device(m, d_sec, d_rec, t_max=t_max)
            b = ctx.last_trace_ms()[0]
            if rep:
                t_any.append(a), t_closest.append(b)
        torch.cuda.synchronize()
        occluded = int(cnt.cpu().numpy()[1])
        ds.occluded_device(groups, N_DIRS, d_sec, out_occluded=d_flags, t_max=t_max)
        torch.cuda.synchronize()
        same = bool(torch.equal(d_flags, (d_rec[:, 0] != 0).to(torch.uint8)))
        res["secondary_" + tag] = {"occluded": _median(t_any), "query_hits": _median(t_closest), "occluded_rays": occluded,
                                   "counts_sum": int(d_count.sum().item()), "flags_are_the_closest_hit_searchs": same,
                                   "any_over_closest": statistics.median(t_any) / statistics.median(t_closest)}

    # (c) how much of the tree each search visits
    if which == "C3":
        ctx.set_option("count_traversal", 1)
        for tag, t_max in (("radius_1", 1.0), ("unbounded", FLT_MAX)):
            ds.occluded_device(groups, N_DIRS, d_sec, out_count=d_count, t_max=t_max)
            any_hit = ctx.last_traversal_counters()
            ds.query_hits_device(m, d_sec, d_rec, t_max=t_max)
            closest = ctx.last_traversal_counters()
            res["counters_" + tag] = {"occluded": {"aabb": any_hit[0], "prim": any_hit[1]}, "query_hits": {"aabb": closest[0], "prim": closest[1]},
                                      "any_over_closest": sum(any_hit) / max(1, sum(closest))}
        ctx.set_option("count_traversal", 0)
    ds.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "visibility"))
    ap.add_argument("--child", default=None, choices=SCENES)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        res = measure(a.child)
        with open(os.path.join(a.out, "visibility_%s.json" % a.child), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res), flush=True)
        return 0
    for which in SCENES:
        print("== visibility, scene %s (limit %d s)" % (which, LIMIT), flush=True)
        try:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--out", a.out], check=True, timeout=LIMIT, cwd=ROOT)
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
            print("the measurement failed: %s" % e, flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
