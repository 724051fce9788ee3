"""Light-sampled frames through participating media, measured: what the shadow rays through the media cost per frame, what
the VOL instantiation itself costs where there is no medium, and what the light samples buy in error on the scenes they were shut out of.

    python scripts/gpu_vol.py [--out DIR] [--only device|error]

One child process per measurement, each under its own time limit; the first failure ends the run.  Every child writes DIR/vol_<name>.json.  A warm-up,
then the median of 5 with minimum - maximum, the compared calls alternated in one process:

  device  device time (RTMI_FLAG_TIMING: the path kernel alone) at 1920 x 1080 x 4, depth 50.  On the smoke Cornell box and make-final:
          rtmi_render_lit_vol_device (MIS, uniform pick) against rtmi_render_lit_device estimator 0 on the same scene -- the same paths without the
          shadow rays.  On the classic Cornell box: against rtmi_render_lit_device estimator 2 -- the same work, so the ratio is what the VOL
          instantiation itself costs.  The ratio is reported beside the yardstick's own min - max spread.
  error   256 x 256 x 16 on the smoke box, 250 x 250 x 16 on make-final, five seeds: RMS error (over pixels and channels, linear radiance) and the
          median over pixels of the absolute error against a 4 096-spp plain frame of the device, of volume-MIS, of the plain estimator at equal
          samples, and of the plain estimator at the samples volume-MIS's device time pays for (equal time)."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.gpu_nee import DEPTH, LIMIT, PER_PIXEL, REFERENCE_SPP, REPS, SPP, VIEW, _median  # noqa: E402  (the NEE measurement's recipes)

SCENES = ("smoke", "final", "classic")
ERROR_FRAMES = {"smoke": 256, "final": 250}
SEEDS = (11, 12, 13, 14, 15)
CHILDREN = tuple("device_%s" % w for w in SCENES) + tuple("error_%s" % w for w in ERROR_FRAMES)


def _scene(which, nx, ny):
    import raytrace_clj_amd as r
    if which == "final":
        return r.scene.make_final(nx, ny)
    return r.scene.make_cornell_box(nx, ny, classic=(which == "classic"))


def measure_device(which):
    import torch

    from raytrace_clj_amd import core
    nx, ny = VIEW
    ctx = core.Context(0, timing=True)
    ds = core.DeviceScene(_scene(which, nx, ny), ctx=ctx)
    ng, n = nx * ny, nx * ny * PER_PIXEL
    yard = 2 if which == "classic" else 0  # the yardstick's estimator: the same work without VOL, or the same paths without shadow rays
    lin = {k: torch.zeros((ny, nx, 3), dtype=torch.float64, device="cuda") for k in ("vol", "yard")}
    err = torch.zeros(ng, dtype=torch.float64, device="cuda")
    cnt = {k: torch.zeros(4, dtype=torch.int64, device="cuda") for k in ("vol", "yard")}
    torch.cuda.synchronize()
    times = {"vol": [], "yard": []}
    for rep in range(REPS + 1):
        ds.render_lit_vol_device(nx, ny, 0, PER_PIXEL, lin["vol"], err, estimator="mis", depth=DEPTH, out_counters=cnt["vol"])
        a = ctx.last_trace_ms()[0]
        ds.render_lit_device(nx, ny, 0, PER_PIXEL, lin["yard"], err, estimator=yard, depth=DEPTH, out_counters=cnt["yard"])
        b = ctx.last_trace_ms()[0]
        if rep:
            times["vol"].append(a), times["yard"].append(b)
        print("rep %d: volume MIS %.2f ms, estimator %d %.2f ms" % (rep, a, yard, b), flush=True)
    torch.cuda.synchronize()
    counters = {k: cnt[k].cpu().numpy().tolist() for k in cnt}
    vol, ys = _median(times["vol"]), _median(times["yard"])
    res = {"scene": which, "view": list(VIEW), "paths": n, "depth": DEPTH, "primitives": int(len(ds.flat.prim_kind)), "lights": ds.lights().tolist(),
           "library": os.path.basename(core._ffi.LIB_PATH), "yardstick_estimator": yard, "counters": counters, "vol": vol, "yardstick": ys,
           "reps_vol_ms": times["vol"], "reps_yardstick_ms": times["yard"], "vol_ns_per_path": vol["median_ms"] * 1e6 / n,
           "vol_over_yardstick": vol["median_ms"] / ys["median_ms"],
           "yardstick_spread_over_median": [ys["min_ms"] / ys["median_ms"], ys["max_ms"] / ys["median_ms"]],
           "within_yardstick_spread": ys["min_ms"] <= vol["median_ms"] <= ys["max_ms"]}
    same_paths = counters["vol"][:2] == counters["yard"][:2] and counters["vol"][1] == n
    res["ok"] = same_paths and (counters["vol"] == counters["yard"] if which == "classic" else counters["vol"][2] > 0)
    if which == "classic":
        res["same_image"] = bool(torch.equal(lin["vol"], lin["yard"]))
        res["ok"] = res["ok"] and res["same_image"]
    ds.close()
    ctx.close()
    return res


def measure_error(which):
    import numpy as np

    from raytrace_clj_amd import core
    side = ERROR_FRAMES[which]
    ctx = core.Context(0, timing=True)
    ds = core.DeviceScene(_scene(which, side, side), ctx=ctx)
    ref = np.zeros((side, side, 3))
    for k, seed in enumerate((901, 902, 903, 904)):  # 4 096 spp as four frames of 1 024 with seeds of their own
        ref += ds.render_lit(side, side, REFERENCE_SPP // 4, estimator="plain", depth=DEPTH, seed=seed)[0] / 4.0
        print("reference part %d" % k, flush=True)

    def stats(lin):
        e = lin - ref
        return float(np.sqrt(np.mean(e * e))), float(np.median(np.abs(e).mean(axis=2)))
    rows = []
    for seed in SEEDS:
        ds.render_lit_vol(side, side, SPP, estimator="mis", depth=DEPTH, seed=seed)  # (a warm-up; the timing window is emptied behind it)
        ctx.last_trace_ms()
        vol = ds.render_lit_vol(side, side, SPP, estimator="mis", depth=DEPTH, seed=seed)
        t_vol = ctx.last_trace_ms()[0]
        plain = ds.render_lit(side, side, SPP, estimator="plain", depth=DEPTH, seed=seed)
        t_plain = ctx.last_trace_ms()[0]
        equal = max(SPP, int(round(SPP * t_vol / t_plain)))
        more = ds.render_lit(side, side, equal, estimator="plain", depth=DEPTH, seed=seed)
        row = {"seed": seed, "vol_ms": t_vol, "plain_ms": t_plain, "equal_time_spp": equal, "vol": stats(vol[0]), "plain": stats(plain[0]),
               "plain_equal_time": stats(more[0]), "counters_vol": vol[3].tolist()}
        rows.append(row)
        print(json.dumps(row), flush=True)
    med = lambda key, k: float(np.median([r[key][k] for r in rows]))
    res = {"scene": which, "frame": [side, side, SPP], "reference_spp": REFERENCE_SPP, "depth": DEPTH, "rows": rows,
           "rms": {k: med(k, 0) for k in ("vol", "plain", "plain_equal_time")}, "median_pixel": {k: med(k, 1) for k in ("vol", "plain", "plain_equal_time")}}
    res["rms_plain_over_vol"] = res["rms"]["plain"] / res["rms"]["vol"]
    res["rms_plain_equal_time_over_vol"] = res["rms"]["plain_equal_time"] / res["rms"]["vol"]
    res["ok"] = all(r["counters_vol"][2] > 0 for r in rows)
    ds.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "vol"))
    ap.add_argument("--only", default=None, choices=("device", "error"))
    ap.add_argument("--child", default=None, choices=CHILDREN)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        kind, which = a.child.split("_", 1)
        res = {"device": measure_device, "error": measure_error}[kind](which)
        with open(os.path.join(a.out, "vol_%s.json" % a.child), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res), flush=True)
        if not res["ok"]:
            print("the compared calls did not do the work they were meant to: the figures compare different things", flush=True)
            return 1
        return 0
    for which in CHILDREN:
        if a.only and not which.startswith(a.only):
            continue
        print("== volume rule, %s (limit %d s)" % (which, LIMIT), flush=True)
        try:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--out", a.out], check=True, timeout=LIMIT, cwd=ROOT)
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
            print("the measurement failed: %s" % e, flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
