"""Direct lighting from first hits, measured: what sampling the lights on the device costs next to tracing the same shadow rays
from HBM, and what the whole pass costs next to the host round trip it replaces.

    python scripts/gpu_direct.py [--out DIR]

One child process per scene, each under its own time limit; the first failure ends the run.  Every child writes DIR/direct_<scene>.json.  The view is
1920 x 1080 with 8 samples per first hit and light; a warm-up, then the median of 5, the compared calls alternated in one process:

  (a) light source  device time (RTMI_FLAG_TIMING: the query kernel alone) of rtmi_direct_irradiance_device -- the SRC_LIGHT launch over every item,
                    which also writes 24 bytes per item for the fold -- against rtmi_query_occluded_device, the parent's way to trace them, on rays
                    resident in HBM, in two forms: the same rows (the call's own out_rays, zeros where an item builds no ray), and the built rays
                    alone, compacted (fewer items than the light source visits).  The fold's own interval is reported beside it.
  (b) whole pass    wall time (a host clock around calls that end synchronised, host arrays out) of DeviceScene.render_direct against the round trip it
                    replaces: first hits downloaded, the shadow rays built in numpy (camera.light_samples), uploaded to occlusion_targets' any-hit
                    search (DeviceScene.occluded), weighted and folded on the host

  scenes: C3 = the cover scene with 10 001 spheres and one added sphere lamp; cornell = the Cornell box
The child fails (exit status 1) if the light source's flags are not the memory source's."""
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

LIMIT = 480  # seconds per scene
REPS = 5
VIEW = (1920, 1080)
N_SAMPLES = 8
SCENES = ("C3", "cornell")


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


def measure(which):
    import numpy as np
    import torch

    from raytrace_clj_amd import _ffi, camera, core
    nx, ny = VIEW
    ctx = core.Context(0, timing=True)
    ds = core.DeviceScene(_scene(which, nx, ny), ctx=ctx)
    f = ds.flat
    n = nx * ny
    lights = ds.lights()
    table = camera.light_table(f, lights)
    nl = len(lights)
    items = n * N_SAMPLES * nl
    res = {"scene": which, "view": list(VIEW), "points": n, "n_samples": N_SAMPLES, "lights": lights.tolist(), "items": items,
           "primitives": int(len(f.prim_kind))}

    # the points: the first hits of the pixel-centre rays, resident
    primary = ds.pixel_centre_rays(nx, ny)
    d_view = torch.from_numpy(primary).cuda()
    d_hits = torch.zeros((n, _ffi.HIT_REC), dtype=torch.float64, device="cuda")
    d_E = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    d_rays = torch.zeros((items, 7), dtype=torch.float64, device="cuda")
    d_flags = torch.zeros(items, dtype=torch.uint8, device="cuda")
    d_flags2 = torch.zeros(items, dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    ds.query_hits_device(n, d_view, d_hits)
    ds.direct_irradiance_device(n, d_hits, N_SAMPLES, d_E, view=d_view, lambert_only=True, out_rays=d_rays, out_occluded=d_flags, out_counters=cnt)
    torch.cuda.synchronize()
    res["points_hit"] = int((d_hits[:, 0] != 0).sum().item())
    res["rays_built"], res["rays_occluded"] = (int(x) for x in cnt.cpu().numpy())

    # (a) the SRC_LIGHT launch over every item against the memory source, in two forms: on the same rows (the call's own out_rays: one row per item, zeros
    # where the item builds no ray -- like for like in items, though a zero direction is a ray no caller would upload), and on the rays that were built
    # alone, compacted (what a caller who builds rays on the host would upload: fewer items than the light source visits)
    built = (d_rays[:, 3:6] != 0).any(dim=1)
    d_some = d_rays[built].contiguous()
    n_some = int(d_some.shape[0])
    torch.cuda.synchronize()
    t_gen, t_fold, t_all, t_some = [], [], [], []
    for rep in range(REPS + 1):
        ds.direct_irradiance_device(n, d_hits, N_SAMPLES, d_E, view=d_view, lambert_only=True)
        a, fold = ctx.last_trace_ms()[0], ctx.last_reduce_ms()[0]
        ds.occluded_device(items, 1, d_rays, out_occluded=d_flags2, t_min=0.001, t_max=1.0 - 0.001)
        b = ctx.last_trace_ms()[0]
        if rep == 0:
            torch.cuda.synchronize()
            same_rows = bool(torch.equal(d_flags, d_flags2))
        ds.occluded_device(n_some, 1, d_some, out_occluded=d_flags2, t_min=0.001, t_max=1.0 - 0.001)
        c = ctx.last_trace_ms()[0]
        if rep:
            t_gen.append(a), t_fold.append(fold), t_all.append(b), t_some.append(c)
    torch.cuda.synchronize()
    same = same_rows and n_some == res["rays_built"] and bool(torch.equal(d_flags[built], d_flags2[:n_some])) and not bool(d_flags[~built].any())
    res["light_source"] = {"generated_source": _median(t_gen), "fold": _median(t_fold), "memory_source_same_rows": _median(t_all),
                           "memory_source_built_rays": _median(t_some), "flags_are_the_memory_sources": same,
                           "generated_over_memory_same_rows": statistics.median(t_gen) / statistics.median(t_all),
                           "generated_over_memory_built_rays": statistics.median(t_gen) / statistics.median(t_some), "built_rays": n_some,
                           "contribution_bytes": items * 24, "ray_bytes_same_rows": items * 56, "ray_bytes_built_rays": n_some * 56}
    del d_rays, d_some, d_flags, d_flags2, built

    # (b) the whole pass against the host round trip
    def round_trip():
        hits = ds.query_hits(primary)
        mat_kind = np.asarray(f.mat_kind)
        lamb = (hits[:, 0] != 0) & (mat_kind[hits[:, 11].astype(np.int64)] == 0)
        normals = hits[:, 6:9].copy()
        away = (normals * primary[:, 3:6]).sum(axis=1) > 0.0
        normals[away] = -normals[away]
        rays, w, built = camera.light_samples(hits[lamb, 3:6], normals[lamb], table, N_SAMPLES, seed=core.RENDER_SEED, time=float(primary[0, 6]))
        flags = np.zeros(len(rays), np.uint8)
        flags[built] = ds.occluded(np.ascontiguousarray(rays[built]), t_min=0.001, t_max=1.0 - 0.001)[0]
        le = table[np.arange(len(w)) % nl, 7:10]
        E = np.zeros((n, 3))
        E[lamb] = (le * (w * (flags == 0))[:, None]).reshape(-1, N_SAMPLES * nl, 3).sum(axis=1) / N_SAMPLES
        return E

    t_old, t_new = [], []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        E = round_trip()
        t1 = time.perf_counter()
        lin = ds.render_direct(nx, ny, N_SAMPLES)[0]
        t2 = time.perf_counter()
        if rep:
            t_old.append((t1 - t0) * 1e3), t_new.append((t2 - t1) * 1e3)
    res["whole_pass_host_round_trip"], res["whole_pass_render_direct"] = _median(t_old), _median(t_new)
    res["whole_pass_new_over_old"] = statistics.median(t_new) / statistics.median(t_old)
    res["mean_irradiance_round_trip"], res["mean_linear_render_direct"] = float(E.mean()), float(lin.mean())
    ds.close()
    ctx.close()
    res["ok"] = same
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "direct"))
    ap.add_argument("--child", default=None, choices=SCENES)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        res = measure(a.child)
        with open(os.path.join(a.out, "direct_%s.json" % a.child), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res), flush=True)
        if not res["ok"]:
            print("the light source's flags are not the memory source's: the timings compare different work", flush=True)
            return 1
        return 0
    for which in SCENES:
        print("== direct lighting, scene %s (limit %d s)" % (which, LIMIT), flush=True)
        try:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--out", a.out], check=True, timeout=LIMIT, cwd=ROOT)
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
            print("the measurement failed: %s" % e, flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
