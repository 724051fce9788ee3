"""Caller-supplied rays on the GPU, measured: what rtmi_render_rays_device costs for the rays of a whole frame next to the
frame kernel that generates the same rays itself, and next to rtmi_probe_paths, the only call that took rays before.

    python scripts/gpu_rays.py [--out DIR]

One child process per scene, each under its own time limit; the first failure ends the run.  Every child writes DIR/rays_<scene>.json.  The frame is
1920 x 1080 x 4 behind a pinhole camera with the scene's image plane (a pinhole path starts at draw 2 of its stream, so one ctr0 serves every ray);
its rays are generated once with probe_camera, grouped per pixel (group j * nx + i, so the keys the library derives are the frame's).  A warm-up,
then the median of 5, by the library's own events (RTMI_FLAG_TIMING):

  rays    rtmi_render_rays_device on those rays, HBM-resident, no per-ray output: trace (rays_kernel) and fold (rays_fold_kernel) ms
  frame   rtmi_render_device of the same frame: trace and reduce ms
  probe   rtmi_probe_paths on the same rays and keys from host arrays: WALL time -- it uploads 64 bytes per ray and reads 36 back per call

  scenes: C3 = the cover scene with 10 001 spheres; glass = the cover scene n = 11 with choose-mat at (0.1, 0.2): four of five small spheres glass
The child also states whether every ray's radiance is the probe's and whether the means of `rays` are the frame's linear image, bit for bit."""
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
FRAME = (1920, 1080, 4)
SCENES = ("C3", "glass")


def _median(samples):
    return {"median_ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples), "n": len(samples)}


def measure(which):
    import numpy as np
    import torch

    import raytrace_clj_amd as r
    from raytrace_clj_amd import camera as cam
    from raytrace_clj_amd import core, util
    nx, ny, ns = FRAME
    sc = r.scene.make_random_scene(nx, ny, 50, False) if which == "C3" else r.scene.make_random_scene(nx, ny, 11, False, mix=(0.1, 0.2))
    lens = sc["camera"]
    ctx = core.Context(0, timing=True)
    ds = core.DeviceScene(sc["world"], camera=cam.PinholeCamera(lens.origin, lens.lleft, lens.horiz, lens.vert), ctx=ctx)
    assert int(ds.flat.cam_kind) == 0
    seed, n = core.RENDER_SEED, nx * ny * ns
    pix, ss = (a.ravel() for a in np.meshgrid(np.arange(nx * ny), np.arange(ns), indexing="ij"))
    keys = util.sample_keys(seed, pix, ss)
    u = ((pix % nx).astype(np.float32).astype(np.float64) + util.draw_uniforms(keys, 0)) / np.float64(nx)
    v = ((pix // nx).astype(np.float32).astype(np.float64) + util.draw_uniforms(keys, 1)) / np.float64(ny)
    rays = np.ascontiguousarray(ds.probe_camera(np.stack([u, v], 1), keys)[:, :7])
    del u, v, pix, ss
    res = {"scene": which, "frame": list(FRAME), "rays": n, "primitives": int(len(ds.flat.prim_kind))}

    d_rays = torch.from_numpy(rays).cuda()
    mean = torch.zeros((nx * ny, 3), dtype=torch.float64, device="cuda")
    err = torch.zeros(nx * ny, dtype=torch.float64, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    lin = torch.zeros((ny, nx, 3), dtype=torch.float64, device="cuda")
    fcnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    t_rays, f_rays, t_frame, f_frame = [], [], [], []
    for rep in range(REPS + 1):  # the two alternate; repetition 0 warms up (workspace, occupancy queries)
        ds.render_rays_device(nx * ny, ns, d_rays, mean, err, seed=seed, ctr0=2, out_counters=cnt)
        a, b = ctx.last_trace_ms()[0], ctx.last_reduce_ms()[0]
        ds.render_device(nx, ny, ns, out_linear=lin, out_counters=fcnt, seed=seed)
        c, d = ctx.last_trace_ms()[0], ctx.last_reduce_ms()[0]
        if rep:
            t_rays.append(a), f_rays.append(b), t_frame.append(c), f_frame.append(d)
    torch.cuda.synchronize()
    res["rays_trace"], res["rays_fold"], res["frame_trace"], res["frame_reduce"] = _median(t_rays), _median(f_rays), _median(t_frame), _median(f_frame)
    res["segments"] = [int(x) for x in cnt.cpu().numpy()]
    res["frame_counters"] = [int(x) for x in fcnt.cpu().numpy()]
    h_mean, h_lin = mean.cpu().numpy().reshape(ny, nx, 3)[::-1], lin.cpu().numpy()
    res["means_are_the_frame"] = bool(np.array_equal(h_mean, h_lin))
    res["pixels_differing"] = int((h_mean != h_lin).any(axis=2).sum())
    out = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ds.render_rays_device(nx * ny, ns, d_rays, mean, err, seed=seed, ctr0=2, out_rays=out, out_counters=cnt)
    torch.cuda.synchronize()
    h_out = out.cpu().numpy()
    del d_rays, mean, err, lin, out
    torch.cuda.empty_cache()

    walls = []
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        rgb, nseg, _, _ = ds.probe_paths(rays, keys, ctr0=2)
        if rep:
            walls.append((time.perf_counter() - t0) * 1e3)
    res["probe_wall"] = _median(walls)
    res["rays_are_the_probes"] = bool(np.array_equal(h_out, rgb))
    res["rays_differing"] = int((h_out != rgb).any(axis=1).sum())
    res["probe_segments"] = int(nseg.sum())
    a, f, p = res["rays_trace"]["median_ms"] + res["rays_fold"]["median_ms"], res["frame_trace"]["median_ms"] + res["frame_reduce"]["median_ms"], res["probe_wall"]["median_ms"]
    res["rays_over_frame"], res["probe_over_rays"] = a / f, p / a
    ds.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "rays"))
    ap.add_argument("--child", default=None, choices=SCENES)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        res = measure(a.child)
        with open(os.path.join(a.out, "rays_%s.json" % a.child), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res), flush=True)
        return 0
    for which in SCENES:
        print("== rays, scene %s (limit %d s)" % (which, LIMIT), flush=True)
        try:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--out", a.out], check=True, timeout=LIMIT, cwd=ROOT)
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
            print("the measurement failed: %s" % e, flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
