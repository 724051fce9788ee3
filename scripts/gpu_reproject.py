"""Temporal accumulation on the GPU, measured.

    python scripts/gpu_reproject.py [--out DIR] [step ...]      steps: time-C3

Every step is a child process of its own under a time limit; the first one that fails (or runs out of time) ends the run, nothing is started after
it.  Each step writes DIR/<step>.json.

  time-C3  1920 x 1080, 10 001 spheres, two pinhole views 1 degree apart taken in turn: the reproject call alone with every test on and with the
           library's defaults; a full accumulator step at 4 spp (camera, frame, features, reproject); the same queue without the reproject call;
           one pass of the denoiser, for scale.  Each timed with device events on one stream after a warm-up, median of 5, alternated in one
           process (the procedure of section 7d)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = {"time-C3": 420}  # step -> time limit in seconds
REPS = 5


def step_time_c3():
    import torch
    import raytrace_clj_amd as r
    from raytrace_clj_amd import camera as cam
    from raytrace_clj_amd import core
    nx, ny, ns, na = 1920, 1080, 4, core.FEATURE_SAMPLES
    ctx = core.Context(0)
    sc = r.scene.make_random_scene(nx, ny, 50, False, mix=(0.8, 0.95))
    ds = core.DeviceScene(sc, ctx=ctx)
    views = cam.orbit(sc["camera"], 360)[:2]
    pairs = [core._camera_pair(c) for c in views]
    f64 = dict(dtype=torch.float64, device="cuda")
    lin, olin, flt = (torch.zeros((ny, nx, 3), **f64) for _ in range(3))
    err, oerr, ow, ferr = (torch.zeros((ny, nx), **f64) for _ in range(4))
    ft = torch.zeros((ny, nx, 8), **f64)
    q = torch.zeros((ny, nx, 3), dtype=torch.uint8, device="cuda")
    cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()  # a stream of torch's own for every call: the events are recorded on it
    st = side.cuda_stream
    acc = core.TemporalAccumulator(ds, nx, ny, ns, na=na, stream=side)
    acc.step(views[0])
    acc.step(views[1])
    # the history the bare call is timed on: the accumulator's own after two steps (view 1), reprojected into view 0
    h = acc._cur
    hist = (acc._lin[h], acc._w[h], acc._se[h], acc._ft[h])
    ds.set_camera(pairs[0], stream=st)
    ds.render_progressive_device(nx, ny, 0, ns, lin, q, err, cnt, stream=st)
    ds.render_features_device(nx, ny, na, ft, None, stream=st)
    side.synchronize()
    turn = [0]

    def bare(outs=None, **kw):
        ctx.reproject_device(nx, ny, pairs[1], pairs[0], *hist, lin, err, ft, float(ns), *(outs or (olin, q, ow, oerr, cnt)), stream=st, **kw)

    def full_step():
        turn[0] += 1
        acc.step(views[turn[0] % 2])

    def step_without_reprojection():
        turn[0] += 1
        ds.set_camera(pairs[turn[0] % 2], stream=st)
        ds.render_progressive_device(nx, ny, 0, ns, lin, q, err, cnt, seed=core.RENDER_SEED + turn[0], stream=st)
        ds.render_features_device(nx, ny, na, ft, None, seed=core.RENDER_SEED + turn[0], stream=st)

    work = {
        "reproject_all_tests": lambda: bare(max_history=32.0, sigma_d=0.05, sigma_n=0.5, sigma_a=0.2),
        "reproject_defaults": lambda: bare(),
        "reproject_defaults_no_rgb8": lambda: bare((olin, None, ow, oerr, cnt)),
        "reproject_defaults_rgb8_only": lambda: bare((None, q, None, None, None)),
        "reproject_defaults_no_counters": lambda: bare((olin, q, ow, oerr, None)),
        "accumulator_step_4spp": full_step,
        "step_without_reprojection_4spp": step_without_reprojection,
        "denoise_1_pass": lambda: ctx.denoise_device(nx, ny, lin, err, ft, flt, q, ferr, iterations=1, stream=st),
    }

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
    bare(max_history=32.0, sigma_d=0.05, sigma_n=0.5, sigma_a=0.2)
    side.synchronize()
    share = [int(v) for v in cnt.cpu().numpy()]
    npx = nx * ny
    out = {"nx": nx, "ny": ny, "spp": ns, "feature_samples": na, "reps": REPS,
           "ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in times.items()},
           "pixels_with_history": share[1] / share[0],
           # per pixel: the current frame's colour, stderr, features (96 B), four taps of colour, weight, stderr, features (4 x 104 B, shared between
           # neighbours through the caches), the outputs: colour, weight, stderr, rgb8 (43 B)
           "bytes": {"compulsory": (96 + 104 + 43) * npx, "requested": (96 + 4 * 104 + 43) * npx}}
    med = out["ms"]["reproject_all_tests"]["median"]
    out["reproject_GBps_compulsory"] = out["bytes"]["compulsory"] / med / 1e6
    for k, v in out["ms"].items():
        print("%-32s median %.3f ms (min %.3f, max %.3f)" % (k, v["median"], v["min"], v["max"]), flush=True)
    print("history on %.3f of the pixels; the bare call moves at least %.0f MB: %.0f GB/s" % (out["pixels_with_history"], out["bytes"]["compulsory"] / 1e6,
                                                                                             out["reproject_GBps_compulsory"]), flush=True)
    ctx.progressive_release()
    ds.close()
    ctx.close()
    return out


CHILD = {"time-C3": step_time_c3}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "reproject"))
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
