"""The feature pass and the denoiser on the GPU, measured.

    python scripts/gpu_denoise.py [--out DIR] [step ...]      steps: grid time-C3 (default: both, in this order)

Every step is a child process of its own under a time limit; the first one that fails (or runs out of time) ends the run, nothing is started after
it.  Each step writes DIR/<step>.json.

  grid     the small cover scene (200 x 100, n = 3) and the Cornell box (128 x 128) at 16 spp against a 4096-spp frame of another seed: RMS error
           of the raw frame and of the filtered frame over a grid of sigmas, five passes, features of 4 samples; the best point per scene, the
           best common point, and what the library's defaults give
  time-C3  1920 x 1080, 10 001 spheres: the feature pass for na = 16, the five-pass filter with the default sigmas (all terms on), and the
           one-shot frame at 256 spp, each timed with device events on one stream after a warm-up, median of 5, alternated in one process;
           the filter's passes also one by one (step 1, 2, 4, 8, 16)"""
import argparse
import itertools
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = {"grid": 420, "time-C3": 420}  # step -> time limit in seconds
REPS = 5


def _rms(a, b):
    import numpy as np
    return float(np.sqrt(np.mean((a - b) ** 2)))


def step_grid():
    import raytrace_clj_amd as r
    from raytrace_clj_amd import core
    ctx = core.Context(0)
    scenes = {"cover": (r.scene.make_random_scene(200, 100, 3, False), 200, 100), "cornell": (r.scene.make_cornell_box(128, 128), 128, 128)}
    grid = {"sigma_c": (0.0, 1.0, 2.0, 4.0, 8.0), "sigma_n": (0.0, 0.25, 0.5), "sigma_a": (0.0, 0.05, 0.1, 0.2), "sigma_d": (0.0, 0.05, 0.2)}
    points = [dict(zip(grid, v)) for v in itertools.product(*grid.values())]
    out = {"grid": grid, "spp": 16, "truth_spp": 4096, "iterations": 5, "feature_samples": core.FEATURE_SAMPLES, "scenes": {}}
    ratios = {}
    for name, (sc, nx, ny) in scenes.items():
        ds = core.DeviceScene(sc, ctx=ctx)
        truth = ds.render(nx, ny, 4096, seed=core.RENDER_SEED + 1)[0]
        lin, _, err, _ = ds.render_progressive(nx, ny, 0, 16)
        ctx.progressive_release()
        ft = ds.render_features(nx, ny, core.FEATURE_SAMPLES)[0]
        raw = _rms(lin, truth)
        ratios[name] = [_rms(ctx.denoise(lin, err, ft, iterations=5, **p)[0], truth) / raw for p in points]
        by_iter = {it: _rms(ctx.denoise(lin, err, ft, iterations=it)[0], truth) / raw for it in range(0, 9)}
        best = min(range(len(points)), key=lambda k: ratios[name][k])
        default = _rms(ctx.denoise(lin, err, ft)[0], truth) / raw
        out["scenes"][name] = {"nx": nx, "ny": ny, "raw_rms": raw, "best": points[best], "best_ratio": ratios[name][best], "default_ratio": default,
                               "default_ratio_by_iterations": by_iter}
        print("%s: raw RMS %.5f; best %s ratio %.3f; defaults ratio %.3f; by passes %s" % (
            name, raw, points[best], ratios[name][best], default, " ".join("%d:%.3f" % kv for kv in by_iter.items())), flush=True)
        ds.close()
    # the common point: the smallest product of the two ratios (their geometric mean)
    score = [ratios["cover"][k] * ratios["cornell"][k] for k in range(len(points))]
    order = sorted(range(len(points)), key=lambda k: score[k])
    out["common"] = [{"sigmas": points[k], "cover": ratios["cover"][k], "cornell": ratios["cornell"][k]} for k in order[:10]]
    for row in out["common"]:
        print("common: %s cover %.3f cornell %.3f" % (row["sigmas"], row["cover"], row["cornell"]), flush=True)
    out["defaults"] = {"iterations": core.DENOISE_ITERATIONS, "sigma_c": core.DENOISE_SIGMA_C, "sigma_n": core.DENOISE_SIGMA_N,
                       "sigma_a": core.DENOISE_SIGMA_A, "sigma_d": core.DENOISE_SIGMA_D}
    ctx.close()
    return out


def step_time_c3():
    import torch
    import raytrace_clj_amd as r
    from raytrace_clj_amd import core
    nx, ny, ns, na = 1920, 1080, 256, 16
    ctx = core.Context(0)
    ds = core.DeviceScene(r.scene.make_random_scene(nx, ny, 50, False, mix=(0.8, 0.95)), ctx=ctx)
    lin = torch.zeros((ny, nx, 3), dtype=torch.float64, device="cuda")
    flt = torch.zeros_like(lin)
    q = torch.zeros((ny, nx, 3), dtype=torch.uint8, device="cuda")
    err = torch.zeros((ny, nx), dtype=torch.float64, device="cuda")
    ferr = torch.zeros_like(err)
    ft = torch.zeros((ny, nx, 8), dtype=torch.float64, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()  # a stream of torch's own for every call: the events are recorded on it
    st = side.cuda_stream
    # the frame the filter is timed on: 16 spp with its noise estimate
    ds.render_progressive_device(nx, ny, 0, 16, lin, q, err, cnt, stream=st)
    side.synchronize()
    ctx.progressive_release()
    work = {
        "features_na16": lambda: ds.render_features_device(nx, ny, na, ft, cnt, stream=st),
        "denoise_5_passes": lambda: ctx.denoise_device(nx, ny, lin, err, ft, flt, q, ferr, stream=st),
        "denoise_0_passes": lambda: ctx.denoise_device(nx, ny, lin, err, ft, flt, q, ferr, iterations=0, stream=st),
        "one_shot_256spp": lambda: ds.render_device(nx, ny, ns, flt, q, cnt, stream=st),
    }
    for it in range(1, 6):
        work["denoise_%d_passes" % it] = (lambda it=it: ctx.denoise_device(nx, ny, lin, err, ft, flt, q, ferr, iterations=it, stream=st))

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(side)
        fn()
        b.record(side)
        b.synchronize()
        return a.elapsed_time(b)

    times = {k: [] for k in work}
    for k, fn in work.items():  # warm-up: code objects, workspace allocations
        timed(fn)
    for rep in range(REPS):
        for k, fn in work.items():
            times[k].append(timed(fn))
    out = {"nx": nx, "ny": ny, "reps": REPS, "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()}}
    med = {k: v["median"] for k, v in out["ms"].items()}
    out["ms_per_pass"] = {"step_%d" % (1 << (it - 1)): med["denoise_%d_passes" % it] - med["denoise_%d_passes" % (it - 1)] for it in range(1, 6)}
    npx = nx * ny
    out["bytes"] = {"planes_with_features": 15 * npx * 8, "features_out": 64 * npx,
                    "tap_reads_per_pass_all_terms": 25 * 11 * 8 * npx}  # what a pass asks the cache hierarchy for, not HBM traffic
    for k, v in out["ms"].items():
        print("%-20s median %.3f ms (min %.3f, max %.3f)" % (k, v["median"], v["min"], v["max"]), flush=True)
    print("per pass:", " ".join("%s %.3f ms" % kv for kv in out["ms_per_pass"].items()), flush=True)
    ds.close()
    ctx.close()
    return out


CHILD = {"grid": step_grid, "time-C3": step_time_c3}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "denoise"))
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    ap.add_argument("steps", nargs="*", default=list(STEPS))
    args = ap.parse_args()
    os.makedirs(args.out, exist_ok=True)
    if args.child:
        res = CHILD[args.child]()
        with open(os.path.join(args.out, args.child + ".json"), "w") as f:
            json.dump(res, f, indent=1)
        return 0
    for step in args.steps:
        if step not in STEPS:
            raise SystemExit("unknown step %r; one of %s" % (step, ", ".join(STEPS)))
    for step in args.steps:
        print("== %s (limit %d s)" % (step, STEPS[step]), flush=True)
        try:
            rc = subprocess.run([sys.executable, os.path.abspath(__file__), "--out", args.out, "--child", step], timeout=STEPS[step]).returncode
        except subprocess.TimeoutExpired:
            print("step %s ran out of time: stopping" % step)
            return 124
        if rc != 0:
            print("step %s failed with status %d: stopping" % (step, rc))
            return rc
    return 0


if __name__ == "__main__":
    sys.exit(main())
