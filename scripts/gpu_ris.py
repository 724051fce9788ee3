"""The proposal rule for the light-sampled paths, measured: what proposing on every lamp costs beside the MIS kernel, and what the
choice does to the error.

    python scripts/gpu_ris.py [--out DIR] [--only paths|error]

One child process per measurement, each under its own time limit; the first failure ends the run.  Every child writes DIR/ris_<name>.json.  A warm-up,
then the median of 5 with minimum - maximum, the compared calls alternated in one process:

  paths  device time (RTMI_FLAG_TIMING: the path kernel alone) of rtmi_render_rays_ris_device against rtmi_render_rays_mis_device (both light choices) on
         1920 x 1080 x 4 pinhole paths, depth 50: cornell = the Cornell box (one lamp: the pure overhead of the loop), lamps8 and lamps32 = the recipes of
         tests/ris_cases.py.  The yardstick is the MIS kernel (uniform pick) of the same session.
  error  lamps8 and lamps32 at 256 x 256, 16 samples per pixel, five seeds, against a 4 096-spp frame of rtmi_render: rtmi_render_lit under the MIS rule
         (both picks) and rtmi_render_lit_ris over the same camera rays: the RMS error at equal samples, the device time of the frame, and RMS^2 x time,
         whose ratio is the ratio of squared errors at equal device time."""
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

CHILDREN = ("paths_cornell", "paths_lamps8", "paths_lamps32", "error_lamps8", "error_lamps32")


def _flat(which, nx, ny):
    from tests import ris_cases as rcs
    return _scene(which, nx, ny) if which == "cornell" else rcs.flat(which)


def measure_paths(which):
    import numpy as np
    import torch

    from raytrace_clj_amd import core
    nx, ny = VIEW
    ctx = core.Context(0, timing=True)
    ds = core.DeviceScene(_flat(which, nx, ny), ctx=ctx)
    ng, n = nx * ny, nx * ny * PER_PIXEL
    d_rays = torch.from_numpy(np.repeat(ds.pixel_centre_rays(nx, ny), PER_PIXEL, axis=0)).cuda()
    names = ("mis_uniform", "mis_power", "ris")
    mean = {k: torch.zeros((ng, 3), dtype=torch.float64, device="cuda") for k in names}
    err = {k: torch.zeros(ng, dtype=torch.float64, device="cuda") for k in names}
    cnt = {k: torch.zeros(4, dtype=torch.int64, device="cuda") for k in names}
    times = {k: [] for k in names}
    for rep in range(REPS + 1):
        got = {}
        for k, choice in (("mis_uniform", 0), ("mis_power", 1)):
            ds.render_rays_mis_device(ng, PER_PIXEL, d_rays, mean[k], err[k], light_choice=choice, depth=DEPTH, out_counters=cnt[k])
            got[k] = ctx.last_trace_ms()[0]
        ds.render_rays_ris_device(ng, PER_PIXEL, d_rays, mean["ris"], err["ris"], depth=DEPTH, out_counters=cnt["ris"])
        got["ris"] = ctx.last_trace_ms()[0]
        if rep:
            for k in names:
                times[k].append(got[k])
        print("rep %d: " % rep + ", ".join("%s %.2f ms" % (k, got[k]) for k in names), flush=True)
    torch.cuda.synchronize()
    counters = {k: cnt[k].cpu().numpy().tolist() for k in names}
    res = {"scene": which, "view": list(VIEW), "paths": n, "depth": DEPTH, "primitives": int(len(ds.flat.prim_kind)), "lights": len(ds.lights()),
           "library": os.path.basename(core._ffi.LIB_PATH), "counters": counters}
    for k in names:
        res[k] = _median(times[k])
        res[k + "_ns_per_path"] = res[k]["median_ms"] * 1e6 / n
        res["mean_" + k] = float(mean[k].mean().item())
        res["mean_stderr_" + k] = float(err[k][torch.isfinite(err[k])].mean().item())
    res["ris_over_mis_uniform"] = res["ris"]["median_ms"] / res["mis_uniform"]["median_ms"]
    res["ris_over_mis_power"] = res["ris"]["median_ms"] / res["mis_power"]["median_ms"]
    res["ok"] = counters["ris"][:2] == counters["mis_uniform"][:2]  # the same paths
    ds.close()
    ctx.close()
    return res


def measure_error(which):
    import numpy as np

    from raytrace_clj_amd import core
    ctx = core.Context(0, timing=True)
    ds = core.DeviceScene(_flat(which, FRAME, FRAME), ctx=ctx)
    reference = ds.render(FRAME, FRAME, REFERENCE_SPP, seed=0xBEEF)[0]
    ctx.last_trace_ms()
    print("reference: %d spp, mean %.4f" % (REFERENCE_SPP, reference.mean()), flush=True)
    kinds = {"mis_uniform": lambda seed: ds.render_lit(FRAME, FRAME, SPP, estimator="mis", light_choice=0, seed=seed),
             "mis_power": lambda seed: ds.render_lit(FRAME, FRAME, SPP, estimator="mis", light_choice=1, seed=seed),
             "ris": lambda seed: ds.render_lit_ris(FRAME, FRAME, SPP, seed=seed)}
    for kind in kinds:
        kinds[kind](1)  # warm-up
    rows = []
    for rep in range(REPS):
        row = {}
        for kind in kinds:
            lin = kinds[kind](100 + rep)[0]
            ms = ctx.last_trace_ms()[0]
            rms = float(np.sqrt(np.mean((lin - reference) ** 2)))
            row.update({"rms_" + kind: rms, "ms_" + kind: ms, "rms2_ms_" + kind: rms * rms * ms, "largest_" + kind: float(lin.max())})
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"scene": which, "frame": [FRAME, FRAME], "reference_spp": REFERENCE_SPP, "spp": SPP, "lights": len(ds.lights()), "reps": rows,
           "mean_reference": float(reference.mean())}
    for key in rows[0]:
        vals = [r[key] for r in rows]
        res[key] = {"median": statistics.median(vals), "min": min(vals), "max": max(vals)}
    for k in ("mis_uniform", "mis_power"):
        res["squared_error_%s_over_ris_equal_samples" % k] = (res["rms_" + k]["median"] / res["rms_ris"]["median"]) ** 2
        res["squared_error_%s_over_ris_equal_time" % k] = res["rms2_ms_" + k]["median"] / res["rms2_ms_ris"]["median"]
    res["ok"] = True
    ds.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "ris"))
    ap.add_argument("--only", default=None, choices=("paths", "error"))
    ap.add_argument("--child", default=None, choices=CHILDREN)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        kind, which = a.child.split("_", 1)
        res = measure_error(which) if kind == "error" else measure_paths(which)
        with open(os.path.join(a.out, "ris_%s.json" % a.child), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps({k: v for k, v in res.items() if k != "reps"}), flush=True)
        if not res["ok"]:
            print("the RIS call did not trace the MIS call's paths: the timings compare different work", flush=True)
            return 1
        return 0
    for which in CHILDREN:
        if a.only and not which.startswith(a.only):
            continue
        print("== RIS %s (limit %d s)" % (which, LIMIT), flush=True)
        try:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--out", a.out], check=True, timeout=LIMIT, cwd=ROOT)
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
            print("the measurement failed: %s" % e, flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
