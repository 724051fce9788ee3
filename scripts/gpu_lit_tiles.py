"""Light-sampled frames over a caller's tile list, measured: what the tile source costs beside the row-major frame call, whether
the frame call moved against another build, and what the adaptive loop buys.

    python scripts/gpu_lit_tiles.py [--out DIR] [--only tiles|frame|loop|retire]

One child process per measurement, each under its own time limit; the first failure ends the run.  Every child writes DIR/lit_tiles_<name>.json.  A
warm-up, then the median of 5 with minimum - maximum, the compared calls alternated in one process; scripts/gpu_nee.py's two scenes (C3 = the cover
scene with 10 001 spheres and one added sphere lamp, cornell = the Cornell box), 1920 x 1080 x 4 paths, depth 50, estimator mis:

  tiles   device time (RTMI_FLAG_TIMING: the path kernel alone, and the fold) of rtmi_render_lit_tiles_device with every tile listed against
          rtmi_render_lit_device: the same paths in tile order and in row-major order, the same frame bit for bit.
  frame   rtmi_render_lit_device alone, twice five repetitions (an A/A pair).  The child uses nothing this change adds, so the same file runs in a
          checkout of another commit (copy it into that tree's scripts/): alternate the two trees' runs and compare their medians with the A/A spread.
  loop    the Cornell box 512 x 512, mis, first 16, chunk 16, cap 256: DeviceScene.refine_lit_adaptive at the first eps of EPS_LADDER that takes between
          a quarter and three quarters of the pixel-samples, and once with denoised=True at the same eps; against the uniform frame at the cap and the
          uniform frame of equal pixel-samples: wall time of the synchronised device work and RMS error against a 4096-spp rtmi_render_lit frame.
  retire  one rtmi_tiles_retire_device call on a 1920 x 1080 map with every tile listed (wall time, the call synchronises its stream)."""
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
CHILDREN = tuple("%s_%s" % (kind, which) for kind in ("tiles", "frame") for which in SCENES) + ("loop_cornell", "retire_map")
LOOP = dict(nx=512, ny=512, first=16, chunk=16, cap=256, reference_spp=4096)
EPS_LADDER = (0.04, 0.02, 0.01, 0.08, 0.005)


def _open(which, nx, ny):
    from raytrace_clj_amd import core
    ctx = core.Context(0, timing=True)
    return ctx, core.DeviceScene(_scene(which, nx, ny), ctx=ctx)


def _frame_buffers(nx, ny, names):
    import torch
    f64 = dict(dtype=torch.float64, device="cuda")
    return {k: dict(lin=torch.zeros((ny, nx, 3), **f64), err=torch.zeros((ny, nx), **f64), cnt=torch.zeros(4, dtype=torch.int64, device="cuda"))
            for k in names}


def measure_tiles(which):
    import torch
    nx, ny = VIEW
    ctx, ds = _open(which, nx, ny)
    n_tiles = ((nx + 7) // 8) * ((ny + 7) // 8)
    tiles = torch.arange(n_tiles, dtype=torch.int32, device="cuda")
    b = _frame_buffers(nx, ny, ("tiles", "frame"))
    torch.cuda.synchronize()
    times = {"tiles": [], "tiles_fold": [], "frame": [], "frame_fold": []}
    for rep in range(REPS + 1):
        ds.render_lit_tiles_device(nx, ny, 0, PER_PIXEL, n_tiles, tiles, b["tiles"]["lin"], b["tiles"]["err"], estimator="mis", depth=DEPTH,
                                   out_counters=b["tiles"]["cnt"])
        t, tf = ctx.last_trace_ms()[0], ctx.last_reduce_ms()[0]
        ds.render_lit_device(nx, ny, 0, PER_PIXEL, b["frame"]["lin"], b["frame"]["err"], estimator="mis", depth=DEPTH, out_counters=b["frame"]["cnt"])
        f, ff = ctx.last_trace_ms()[0], ctx.last_reduce_ms()[0]
        if rep:
            times["tiles"].append(t), times["tiles_fold"].append(tf), times["frame"].append(f), times["frame_fold"].append(ff)
        print("rep %d: tile order %.2f + %.2f ms, row-major %.2f + %.2f ms" % (rep, t, tf, f, ff), flush=True)
    torch.cuda.synchronize()
    res = {"scene": which, "view": list(VIEW), "paths": nx * ny * PER_PIXEL, "rows_dealt": n_tiles * 64 * PER_PIXEL, "depth": DEPTH}
    res.update({k: _median(v) for k, v in times.items()})
    res["tiles_over_frame"] = res["tiles"]["median_ms"] / res["frame"]["median_ms"]
    res["frame_spread_over_median"] = [res["frame"]["min_ms"] / res["frame"]["median_ms"], res["frame"]["max_ms"] / res["frame"]["median_ms"]]
    res["counters"] = {k: v["cnt"].cpu().numpy().tolist() for k, v in b.items()}
    res["ok"] = bool(torch.equal(b["tiles"]["lin"], b["frame"]["lin"])) and res["counters"]["tiles"] == res["counters"]["frame"]  # the same frame
    ds.close()
    ctx.close()
    return res


def measure_frame(which):
    import torch

    from raytrace_clj_amd import core
    nx, ny = VIEW
    ctx, ds = _open(which, nx, ny)
    b = _frame_buffers(nx, ny, ("frame",))["frame"]
    torch.cuda.synchronize()
    times = {"a": [], "b": []}
    for rep in range(2 * REPS + 1):
        ds.render_lit_device(nx, ny, 0, PER_PIXEL, b["lin"], b["err"], estimator="mis", depth=DEPTH, out_counters=b["cnt"])
        t = ctx.last_trace_ms()[0]
        if rep:
            times["ab"[rep % 2]].append(t)
        print("rep %d: %.2f ms" % (rep, t), flush=True)
    torch.cuda.synchronize()
    res = {"scene": which, "view": list(VIEW), "paths": nx * ny * PER_PIXEL, "depth": DEPTH, "library": os.path.abspath(core._ffi.LIB_PATH),
           "a": _median(times["a"]), "b": _median(times["b"]), "all": _median(times["a"] + times["b"]), "counters": b["cnt"].cpu().numpy().tolist()}
    res["a_over_b"] = res["a"]["median_ms"] / res["b"]["median_ms"]
    res["ok"] = res["counters"][1] == nx * ny * PER_PIXEL
    ds.close()
    ctx.close()
    return res


def measure_loop(which):
    import numpy as np
    import torch
    nx, ny, first, chunk, cap = (LOOP[k] for k in ("nx", "ny", "first", "chunk", "cap"))
    ctx, ds = _open(which, nx, ny)
    kw = dict(estimator="mis", depth=DEPTH)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3

    def uniform(ns):  # the frame call refined through one state, chunk samples at a time, buffers resident
        f64 = dict(dtype=torch.float64, device="cuda")
        lin, err, state = torch.zeros((ny, nx, 3), **f64), torch.zeros((ny, nx), **f64), torch.zeros((nx * ny, 10), **f64)
        torch.cuda.synchronize()
        k = 0
        while k < ns:
            n = min(chunk, ns - k)
            ds.render_lit_device(nx, ny, k, n, lin, err, state=state, **kw)
            k += n
        torch.cuda.synchronize()
        return lin.cpu().numpy()
    ref = ds.render_lit(nx, ny, LOOP["reference_spp"], chunk=256, **kw)[0]
    rms = lambda a: float(np.sqrt(np.mean((a - ref) ** 2)))  # noqa: E731
    ds.refine_lit_adaptive(nx, ny, 2 * chunk, chunk, 1.0, first=first, **kw)  # warm-up
    ladder, chosen = [], None
    for eps in EPS_LADDER:
        out, ms = timed(lambda: ds.refine_lit_adaptive(nx, ny, cap, chunk, eps, first=first, **kw))
        share = float(out[3].sum()) / (nx * ny * cap)
        ladder.append({"eps": eps, "share": share, "ms": ms, "rounds": len(out[5]), "rms": rms(out[0])})
        print("eps %g: %.1f %% of the pixel-samples, %.1f ms, RMS %.4f" % (eps, 100 * share, ms, ladder[-1]["rms"]), flush=True)
        if 0.25 <= share <= 0.75:
            chosen = ladder[-1]
            break
    res = {"scene": which, "loop": LOOP, "depth": DEPTH, "ladder": ladder, "ok": chosen is not None}
    if chosen:
        eps, equal = chosen["eps"], max(1, int(round(chosen["share"] * cap)))
        runs = {"adaptive": [], "denoised": [], "uniform_cap": [], "uniform_equal": []}
        last = {}
        for rep in range(3):
            for name, f in (("adaptive", lambda: ds.refine_lit_adaptive(nx, ny, cap, chunk, eps, first=first, **kw)),
                            ("denoised", lambda: ds.refine_lit_adaptive(nx, ny, cap, chunk, eps, first=first, denoised=True, **kw)),
                            ("uniform_cap", lambda: uniform(cap)), ("uniform_equal", lambda: uniform(equal))):
                last[name], ms = timed(f)
                runs[name].append(ms)
        res.update({"eps": eps, "equal_spp": equal, "ms": {k: _median(v) for k, v in runs.items()},
                    "rms": {"adaptive": rms(last["adaptive"][0]), "denoised_raw_frame": rms(last["denoised"][0]), "uniform_cap": rms(last["uniform_cap"]),
                            "uniform_equal": rms(last["uniform_equal"])},
                    "share": {"adaptive": chosen["share"], "denoised": float(last["denoised"][3].sum()) / (nx * ny * cap)},
                    "rounds": {"adaptive": [[k, len(t)] for k, t in last["adaptive"][5]], "denoised": [[k, len(t)] for k, t in last["denoised"][5]]}})
    ds.close()
    ctx.close()
    return res


def measure_retire(_which):
    import torch

    from raytrace_clj_amd import core
    nx, ny = VIEW
    ctx = core.Context(0)
    n_tiles = ((nx + 7) // 8) * ((ny + 7) // 8)
    noise = torch.rand((ny, nx), dtype=torch.float64, device="cuda")
    times, kept = [], 0
    for rep in range(REPS + 1):
        tiles = torch.arange(n_tiles, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        kept = ctx.tiles_retire_device(nx, ny, noise, 0.999, n_tiles, tiles)
        ms = (time.perf_counter() - t0) * 1e3
        if rep:
            times.append(ms)
        print("rep %d: %.3f ms, %d of %d tiles kept" % (rep, ms, kept, n_tiles), flush=True)
    res = {"view": list(VIEW), "tiles": n_tiles, "kept": kept, "retire": _median(times), "ok": 0 < kept < n_tiles}
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "lit_tiles"))
    ap.add_argument("--only", default=None, choices=("tiles", "frame", "loop", "retire"))
    ap.add_argument("--child", default=None, choices=CHILDREN)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        kind, which = a.child.split("_", 1)
        res = {"tiles": measure_tiles, "frame": measure_frame, "loop": measure_loop, "retire": measure_retire}[kind](which)
        with open(os.path.join(a.out, "lit_tiles_%s.json" % a.child), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res), flush=True)
        if not res["ok"]:
            print("the measurement did not meet its own condition (see \"ok\" in the code): the figures are not to be used", flush=True)
            return 1
        return 0
    for which in CHILDREN:
        if a.only and not which.startswith(a.only):
            continue
        print("== lit tiles, %s (limit %d s)" % (which, LIMIT), flush=True)
        try:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--out", a.out], check=True, timeout=LIMIT, cwd=ROOT)
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
            print("the measurement failed: %s" % e, flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
