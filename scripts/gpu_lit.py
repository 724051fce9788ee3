"""Light-sampled frames from the scene's camera, measured: what building the camera rays on the device costs beside reading
them, and what the call saves over the round trip it replaces.

    python scripts/gpu_lit.py [--out DIR] [--only device|wall|plain]

One child process per measurement, each under its own time limit; the first failure ends the run.  Every child writes DIR/lit_<name>.json.  A warm-up,
then the median of 5 with minimum - maximum, the compared calls alternated in one process; 1920 x 1080 x 4 paths, depth 50, on scripts/gpu_nee.py's two
scenes (C3 = the cover scene with 10 001 spheres and one added sphere lamp, cornell = the Cornell box):

  device  device time (RTMI_FLAG_TIMING: the path kernel alone) of rtmi_render_lit_device (MIS, uniform pick) against rtmi_render_rays_mis_device on
          the SAME camera rays resident in HBM -- the first call's out_camera, with the frame's keys uploaded beside them.  A rays call starts every
          stream at one ctr0 (the most frequent position behind the camera is taken), so a minority of its paths continue from another draw than the
          frame's: the same work statistically, both counter sets are reported.  The yardstick is the rays call of the same session: the ratio is
          reported beside its own min - max spread, and "within_rays_spread" says whether the new call's median lies inside it.
  wall    wall time of DeviceScene.render_lit (MIS) against DeviceScene.render_nee(mis=True) for the same frame: the host-built rays, the
          rtmi_probe_camera round trip and the upload it replaces.
  plain   for information: estimator 0 (rays_kernel building camera rays, then the fold) against rtmi_render_device (trace_kernel and its fold) for the
          same frame -- the same image; trace_kernel stays the flagship."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.gpu_nee import DEPTH, LIMIT, PER_PIXEL, REPS, VIEW, _median, _scene  # noqa: E402  (the NEE measurement's recipes)

SCENES = ("C3", "cornell")
CHILDREN = tuple("%s_%s" % (kind, which) for kind in ("device", "wall", "plain") for which in SCENES)


def _open(which):
    from raytrace_clj_amd import core
    ctx = core.Context(0, timing=True)
    return ctx, core.DeviceScene(_scene(which, *VIEW), ctx=ctx)


def measure_device(which):
    import numpy as np
    import torch

    from raytrace_clj_amd import core, util
    nx, ny = VIEW
    ctx, ds = _open(which)
    ng, n = nx * ny, nx * ny * PER_PIXEL
    mean = {k: torch.zeros((ng, 3), dtype=torch.float64, device="cuda") for k in ("lit", "rays")}
    err = torch.zeros(ng, dtype=torch.float64, device="cuda")
    cnt = {k: torch.zeros(4, dtype=torch.int64, device="cuda") for k in ("lit", "rays")}
    cam = torch.zeros((n, 8), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    ds.render_lit_device(nx, ny, 0, PER_PIXEL, mean["lit"], err, estimator="mis", depth=DEPTH, out_camera=cam, out_counters=cnt["lit"])
    torch.cuda.synchronize()
    ctx.last_trace_ms()
    d_rays = cam[:, :7].contiguous()
    positions, counts = np.unique(cam[:, 7].cpu().numpy().astype(np.int64), return_counts=True)
    ctr0 = int(positions[counts.argmax()])
    del cam
    y, x, s = (a.ravel() for a in np.meshgrid(np.arange(ny), np.arange(nx), np.arange(PER_PIXEL), indexing="ij"))
    d_keys = torch.from_numpy(util.sample_keys(core.RENDER_SEED, (ny - 1 - y) * nx + x, s).view(np.int64)).cuda()
    torch.cuda.synchronize()
    times = {"lit": [], "rays": []}
    for rep in range(REPS + 1):
        ds.render_lit_device(nx, ny, 0, PER_PIXEL, mean["lit"], err, estimator="mis", depth=DEPTH, out_counters=cnt["lit"])
        a = ctx.last_trace_ms()[0]
        ds.render_rays_mis_device(ng, PER_PIXEL, d_rays, mean["rays"], err, keys=d_keys, ctr0=ctr0, depth=DEPTH, out_counters=cnt["rays"])
        b = ctx.last_trace_ms()[0]
        if rep:
            times["lit"].append(a), times["rays"].append(b)
        print("rep %d: camera rays built %.2f ms, read %.2f ms" % (rep, a, b), flush=True)
    torch.cuda.synchronize()
    counters = {k: cnt[k].cpu().numpy().tolist() for k in cnt}
    lit, rays = _median(times["lit"]), _median(times["rays"])
    res = {"scene": which, "view": list(VIEW), "paths": n, "depth": DEPTH, "primitives": int(len(ds.flat.prim_kind)), "lights": ds.lights().tolist(),
           "library": os.path.basename(core._ffi.LIB_PATH), "counters": counters, "ctr0_of_the_rays_call": ctr0,
           "share_of_paths_at_ctr0": float(counts.max() / counts.sum()), "lit": lit, "rays": rays, "lit_ns_per_path": lit["median_ms"] * 1e6 / n,
           "rays_ns_per_path": rays["median_ms"] * 1e6 / n, "lit_over_rays": lit["median_ms"] / rays["median_ms"],
           "within_rays_spread": rays["min_ms"] <= lit["median_ms"] <= rays["max_ms"], "below_rays_spread": lit["median_ms"] < rays["min_ms"],
           "rays_spread_over_median": [rays["min_ms"] / rays["median_ms"], rays["max_ms"] / rays["median_ms"]],
           "mean_lit": float(mean["lit"].mean().item()), "mean_rays": float(mean["rays"].mean().item())}
    res["ok"] = counters["lit"][1] == counters["rays"][1] == n and abs(counters["lit"][0] - counters["rays"][0]) <= 0.01 * counters["rays"][0]
    ds.close()
    ctx.close()
    return res


def measure_wall(which):
    import numpy as np

    nx, ny = VIEW
    ctx, ds = _open(which)
    times = {"lit": [], "nee": []}
    for rep in range(REPS + 1):
        t0 = time.perf_counter()
        a = ds.render_lit(nx, ny, PER_PIXEL, estimator="mis", depth=DEPTH)
        t1 = time.perf_counter()
        b = ds.render_nee(nx, ny, PER_PIXEL, PER_PIXEL, depth=DEPTH, mis=True)
        t2 = time.perf_counter()
        if rep:
            times["lit"].append((t1 - t0) * 1e3), times["nee"].append((t2 - t1) * 1e3)
        print("rep %d: render_lit %.1f ms, render_nee(mis=True) %.1f ms" % (rep, (t1 - t0) * 1e3, (t2 - t1) * 1e3), flush=True)
    lit, nee = _median(times["lit"]), _median(times["nee"])
    res = {"scene": which, "view": list(VIEW), "samples": PER_PIXEL, "depth": DEPTH, "render_lit": lit, "render_nee_mis": nee,
           "nee_over_lit": nee["median_ms"] / lit["median_ms"], "counters_lit": a[3].tolist(), "counters_nee": b[3].tolist(),
           "mean_lit": float(np.mean(a[0])), "mean_nee": float(np.mean(b[0]))}
    res["ok"] = int(a[3][1]) == int(b[3][1]) == nx * ny * PER_PIXEL
    ds.close()
    ctx.close()
    return res


def measure_plain(which):
    import torch

    nx, ny = VIEW
    ctx, ds = _open(which)
    ng = nx * ny
    lin = {k: torch.zeros((ny, nx, 3), dtype=torch.float64, device="cuda") for k in ("lit", "render")}
    err = torch.zeros(ng, dtype=torch.float64, device="cuda")
    cnt = {"lit": torch.zeros(4, dtype=torch.int64, device="cuda"), "render": torch.zeros(2, dtype=torch.int64, device="cuda")}
    torch.cuda.synchronize()
    times = {"lit": [], "lit_fold": [], "render": [], "render_fold": []}
    for rep in range(REPS + 1):
        ds.render_lit_device(nx, ny, 0, PER_PIXEL, lin["lit"], err, estimator="plain", depth=DEPTH, out_counters=cnt["lit"])
        a, af = ctx.last_trace_ms()[0], ctx.last_reduce_ms()[0]
        ds.render_device(nx, ny, PER_PIXEL, lin["render"], None, cnt["render"], depth=DEPTH)
        b, bf = ctx.last_trace_ms()[0], ctx.last_reduce_ms()[0]
        if rep:
            times["lit"].append(a), times["lit_fold"].append(af), times["render"].append(b), times["render_fold"].append(bf)
        print("rep %d: estimator 0 %.2f + %.2f ms, rtmi_render_device %.2f + %.2f ms" % (rep, a, af, b, bf), flush=True)
    torch.cuda.synchronize()
    res = {"scene": which, "view": list(VIEW), "samples": PER_PIXEL, "depth": DEPTH}
    res.update({k: _median(v) for k, v in times.items()})
    res["lit_over_render"] = (res["lit"]["median_ms"] + res["lit_fold"]["median_ms"]) / (res["render"]["median_ms"] + res["render_fold"]["median_ms"])
    res["counters"] = {k: v.cpu().numpy().tolist() for k, v in cnt.items()}
    res["ok"] = bool(torch.equal(lin["lit"], lin["render"])) and res["counters"]["lit"][0] == res["counters"]["render"][0]  # the same image
    ds.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "lit"))
    ap.add_argument("--only", default=None, choices=("device", "wall", "plain"))
    ap.add_argument("--child", default=None, choices=CHILDREN)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        kind, which = a.child.split("_", 1)
        res = {"device": measure_device, "wall": measure_wall, "plain": measure_plain}[kind](which)
        with open(os.path.join(a.out, "lit_%s.json" % a.child), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res), flush=True)
        if not res["ok"]:
            print("the compared calls did not do the same work: the timings compare different things", flush=True)
            return 1
        return 0
    for which in CHILDREN:
        if a.only and not which.startswith(a.only):
            continue
        print("== lit frames, %s (limit %d s)" % (which, LIMIT), flush=True)
        try:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--out", a.out], check=True, timeout=LIMIT, cwd=ROOT)
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
            print("the measurement failed: %s" % e, flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
