"""What the tile records, the gather and the assemble add to a chunk of an adaptive frame.

    python scripts/gpu_multi_progressive.py [--out DIR] [step ...]      steps: time-C3 (the default)

Every step is a child process of its own under a time limit; the first one that fails (or runs out of time) ends the run, nothing is started after
it.  Each step writes DIR/<step>.json.

  time-C3  1920 x 1080, 10 001 spheres, one chunk of 64 samples into a NEW frame per timed call (s_first = 0: every tile is active), eps = 0 so
           that no tile retires, outputs resident in HBM, in one process, warmed up, median of 5, the three alternated:
             (a) rtmi_render_adaptive_device on one context             -- the single-context path as it was
             (b) rtmi_render_multi_adaptive_device with one replica      -- records, no gather, assemble
             (c) the same with replicas [0, 0]                           -- two contexts sharing the GPU: control flow only, NOT a scaling figure
           Every one of these calls ends with its streams synchronised, so the interval is taken between two device events recorded on an
           otherwise idle stream before and after the call (and the host's clock beside it).  (b) / (a) is the figure that matters."""
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

STEPS = {"time-C3": 420}  # step -> time limit in seconds
REPS = 5


def step_time_c3():
    import numpy as np
    import torch
    import raytrace_clj_amd as r
    from raytrace_clj_amd import core, dist
    nx, ny, chunk, eps = 1920, 1080, 64, 0.0
    flat = r.flatten.flatten(r.scene.make_random_scene(nx, ny, 50, False, mix=(0.8, 0.95)))
    ctx = core.Context(0)
    ds = core.DeviceScene(flat, ctx=ctx)
    one = dist.MultiDevice(flat, [0])
    two = dist.MultiDevice(flat, [0, 0])

    def buffers():
        return (torch.zeros((ny, nx, 3), dtype=torch.float64, device="cuda"), torch.zeros((ny, nx, 3), dtype=torch.uint8, device="cuda"),
                torch.zeros((ny, nx), dtype=torch.float64, device="cuda"), torch.zeros((ny, nx), dtype=torch.int32, device="cuda"),
                torch.zeros(2, dtype=torch.int64, device="cuda"))

    out_a, out_b, out_c = buffers(), buffers(), buffers()
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    work = {
        "a_single_context": lambda: ds.render_adaptive_device(nx, ny, 0, chunk, eps, *out_a),
        "b_multi_one_replica": lambda: one.render_adaptive_device(nx, ny, 0, chunk, eps, *out_b),
        "c_multi_two_replicas_one_gpu": lambda: two.render_adaptive_device(nx, ny, 0, chunk, eps, *out_c),
    }

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record(side)
        fn()
        b.record(side)
        b.synchronize()
        return a.elapsed_time(b), (time.perf_counter() - t0) * 1e3

    for fn in work.values():  # warm-up: code objects, workspace and frame allocations
        timed(fn)
    ev, wall = {k: [] for k in work}, {k: [] for k in work}
    for rep in range(REPS):
        for k, fn in work.items():
            e, w = timed(fn)
            ev[k].append(e)
            wall[k].append(w)
    torch.cuda.synchronize()
    same = all(torch.equal(x, y) and torch.equal(x, z) for x, y, z in zip(out_a, out_b, out_c))
    active = {"a": ctx.adaptive_status()[0], "b": one.adaptive_status()[0], "c": two.adaptive_status()[0]}
    out = {"nx": nx, "ny": ny, "chunk": chunk, "eps": eps, "reps": REPS, "outputs_identical": bool(same), "active_tiles_after": active,
           "tiles": dist.n_tiles(nx, ny), "gather_path": {"b": one.last_gather_path(), "c": two.last_gather_path()},
           "event_ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in ev.items()},
           "wall_ms": {k: {"median": statistics.median(v), "min": min(v), "max": max(v)} for k, v in wall.items()}}
    med = {k: v["median"] for k, v in out["event_ms"].items()}
    out["b_over_a"] = med["b_multi_one_replica"] / med["a_single_context"]
    out["c_over_a"] = med["c_multi_two_replicas_one_gpu"] / med["a_single_context"]
    out["record_bytes"] = int(dist.n_tiles(nx, ny)) * 64 * 5 * 8
    for k, v in out["event_ms"].items():
        print("%-30s median %.3f ms (min %.3f, max %.3f); host clock median %.3f ms" % (k, v["median"], v["min"], v["max"], out["wall_ms"][k]["median"]),
              flush=True)
    print("(b) / (a) = %.4f   (c) / (a) = %.4f   outputs identical: %s   active tiles after: %s of %d" % (
        out["b_over_a"], out["c_over_a"], same, active, out["tiles"]), flush=True)
    assert same, "the three paths must return the same bytes"
    assert int(np.unique(list(active.values())).size) == 1
    two.close()
    one.close()
    ds.close()
    ctx.close()
    return out


CHILD = {"time-C3": step_time_c3}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "multi_progressive"))
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
