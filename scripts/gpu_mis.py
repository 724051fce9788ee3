"""Multiple importance sampling for the light-sampled paths, measured: what the weights cost beside the NEE kernel, and what they
do to the error's tail.

    python scripts/gpu_mis.py [--out DIR] [--only paths|error]

One child process per measurement, each under its own time limit; the first failure ends the run.  Every child writes DIR/mis_<name>.json.  A warm-up,
then the median of 5 with minimum - maximum, the compared calls alternated in one process:

  paths  device time (RTMI_FLAG_TIMING: the path kernel alone) of rtmi_render_rays_mis_device (both light choices) against rtmi_render_rays_nee_device on
         scripts/gpu_nee.py's rays and scenes: 1920 x 1080 x 4 pinhole paths, depth 50; C3 = the cover scene with 10 001 spheres and one added sphere
         lamp, cornell = the Cornell box.  The yardstick is the NEE kernel of the same session: the ratio is reported beside the NEE side's own
         min - max spread, and "within_nee_spread" says whether the MIS median lies inside it.
  error  section 7o's quality table with MIS columns: the Cornell box at 256 x 256, 16 samples per pixel, five seeds, against a 4 096-spp frame of
         rtmi_render; plain, NEE and MIS (both choices) over the same camera rays (DeviceScene.render_nee): the median over pixels of the absolute
         error, the RMS error, the share of the squared error held by the worst 0.1 % of the pixels, each as median (min - max) over the seeds."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.gpu_nee import DEPTH, FRAME, LIMIT, PER_PIXEL, REFERENCE_SPP, REPS, SPP, VIEW, _median, _scene  # noqa: E402  (the NEE measurement's recipes)

CHILDREN = ("paths_C3", "paths_cornell", "error")


def measure_paths(which):
    import numpy as np
    import torch

    from raytrace_clj_amd import core
    nx, ny = VIEW
    ctx = core.Context(0, timing=True)
    ds = core.DeviceScene(_scene(which, nx, ny), ctx=ctx)
    ng, n = nx * ny, nx * ny * PER_PIXEL
    d_rays = torch.from_numpy(np.repeat(ds.pixel_centre_rays(nx, ny), PER_PIXEL, axis=0)).cuda()
    names = ("nee", "mis_uniform", "mis_power")
    mean = {k: torch.zeros((ng, 3), dtype=torch.float64, device="cuda") for k in names}
    err = torch.zeros(ng, dtype=torch.float64, device="cuda")
    cnt = {k: torch.zeros(4, dtype=torch.int64, device="cuda") for k in names}
    times = {k: [] for k in names}
    for rep in range(REPS + 1):
        got = {}
        ds.render_rays_nee_device(ng, PER_PIXEL, d_rays, mean["nee"], err, depth=DEPTH, out_counters=cnt["nee"])
        got["nee"] = ctx.last_trace_ms()[0]
        for k, choice in (("mis_uniform", 0), ("mis_power", 1)):
            ds.render_rays_mis_device(ng, PER_PIXEL, d_rays, mean[k], err, light_choice=choice, depth=DEPTH, out_counters=cnt[k])
            got[k] = ctx.last_trace_ms()[0]
        if rep:
            for k in names:
                times[k].append(got[k])
        print("rep %d: " % rep + ", ".join("%s %.2f ms" % (k, got[k]) for k in names), flush=True)
    torch.cuda.synchronize()
    counters = {k: cnt[k].cpu().numpy().tolist() for k in names}
    res = {"scene": which, "view": list(VIEW), "paths": n, "depth": DEPTH, "primitives": int(len(ds.flat.prim_kind)), "lights": ds.lights().tolist(),
           "library": os.path.basename(core._ffi.LIB_PATH), "counters": counters}
    nee = _median(times["nee"])
    for k in names:
        res[k] = _median(times[k])
        res[k + "_ns_per_path"] = res[k]["median_ms"] * 1e6 / n
        res["mean_" + k] = float(mean[k].mean().item())
    for k in names[1:]:
        res[k + "_over_nee"] = res[k]["median_ms"] / nee["median_ms"]
        res[k + "_within_nee_spread"] = nee["min_ms"] <= res[k]["median_ms"] <= nee["max_ms"]
    res["nee_spread_over_median"] = [nee["min_ms"] / nee["median_ms"], nee["max_ms"] / nee["median_ms"]]
    res["ok"] = counters["mis_uniform"] == counters["nee"] and counters["mis_power"][:2] == counters["nee"][:2]  # the same paths, the same shadow rays
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

    def mae(frame):  # the median over pixels of the absolute error of the channel sum
        return float(np.median(np.abs((frame - reference).sum(axis=2))))

    def worst(frame):  # the share of the squared error that the worst 0.1 % of the pixels hold
        e = np.sort(((frame - reference) ** 2).sum(axis=2).ravel())
        return float(e[-max(1, len(e) // 1000):].sum() / e.sum())

    kinds = {"plain": dict(lights=[]), "nee": dict(), "mis_uniform": dict(mis=True, light_choice=0), "mis_power": dict(mis=True, light_choice=1)}

    def frame(kind, seed):
        lin = ds.render_nee(FRAME, FRAME, SPP, min(SPP, 16), seed=seed, **kinds[kind])[0]
        return lin, ctx.last_trace_ms()[0]
    for kind in kinds:
        frame(kind, 1)  # warm-up
    rows = []
    for rep in range(REPS):
        row = {}
        for kind in kinds:
            lin, ms = frame(kind, 100 + rep)  # section 7o's seeds
            row.update({"rms_" + kind: rms(lin), "median_abs_" + kind: mae(lin), "worst_permille_share_" + kind: worst(lin), "ms_" + kind: ms,
                        "largest_" + kind: float(lin.max())})
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"scene": "cornell", "frame": [FRAME, FRAME], "reference_spp": REFERENCE_SPP, "spp": SPP, "reps": rows, "mean_reference": float(reference.mean())}
    for key in rows[0]:
        vals = [r[key] for r in rows]
        res[key] = {"median": statistics.median(vals), "min": min(vals), "max": max(vals)}
    res["rms_mis_below_plain_every_seed"] = all(r["rms_mis_uniform"] < r["rms_plain"] for r in rows)
    res["ok"] = True
    ds.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "mis"))
    ap.add_argument("--only", default=None, choices=("paths", "error"))
    ap.add_argument("--child", default=None, choices=CHILDREN)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        res = measure_error() if a.child == "error" else measure_paths(a.child.split("_", 1)[1])
        with open(os.path.join(a.out, "mis_%s.json" % a.child), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({k: v for k, v in res.items() if k != "reps"}), flush=True)
        if not res["ok"]:
            print("the MIS call did not trace the NEE call's paths: the timings compare different work", flush=True)
            return 1
        return 0
    for which in CHILDREN:
        if a.only and not which.startswith(a.only):
            continue
        print("== MIS paths, %s (limit %d s)" % (which, LIMIT), flush=True)
        try:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--out", a.out], check=True, timeout=LIMIT, cwd=ROOT)
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
            print("the measurement failed: %s" % e, flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
