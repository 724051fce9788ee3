"""Moving the camera of a live scene on the GPU, measured: what rtmi_scene_set_camera* costs next to creating the scene anew.

    python scripts/gpu_camera.py [--out DIR] [step ...]      steps: set-camera orbit (default: both, in this order)

Every step is a child process of its own under a time limit; the first one that fails (or runs out of time) ends the run, nothing is started after
it.  Each step writes DIR/<step>.json.  One process per step, a warm-up, the median of 5 repetitions, the compared variants alternated inside every
repetition; wall clock around host calls (the stream is idle when the clock starts and synchronised before it stops), device events around work
that is only queued.

  set-camera  C3 (1920x1080's scene: 10 001 spheres) and the Cornell box: creating the scene (DeviceScene(...), the only way before: flattening is
              outside the clock) against set_camera on the fast path -- the host form, and the stream form as host time per call and as device
              time per call (events around 64 queued calls); the moving cover scene (C2m): set_camera on the slow path (two cameras whose shutters
              are disjoint, alternated: every call rebuilds) against creating it
  orbit       the cover scene (C2: 800x400, 64 spp), 32 views about the look-at axis, per view: create + render + destroy; set_camera + render
              (host form, one synchronisation per view); render_views (stream form, one synchronisation per orbit); FramePipeline(depth=2).step
              with cameras (two frames in flight, one synchronisation per orbit)"""
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

STEPS = {"set-camera": 420, "orbit": 300}  # step -> time limit in seconds
REPS = 5
VIEWS = 32


def _median_ms(samples):
    return {"median_ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples), "n": len(samples)}


def _wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def _scene(which):
    import raytrace_clj_amd as r
    if which == "C3":
        return r.scene.make_random_scene(1920, 1080, 50, False)
    if which == "CB":
        return r.scene.make_cornell_box(600, 600)
    if which == "C2m":
        return r.scene.make_random_scene(800, 400, 11, True)
    return r.scene.make_random_scene(800, 400, 11, False)


def _with_camera(flat, camera):
    import copy
    from raytrace_clj_amd import flatten as fl
    f = copy.copy(flat)
    f.cam_kind, f.cam = fl.flatten_camera(camera)
    return f


def _fast_path(which):
    """create against the two fast forms of set_camera, alternated"""
    import torch
    from raytrace_clj_amd import camera as cam, core, flatten as fl
    sc = _scene(which)
    flat = fl.flatten(sc)
    views = cam.orbit(sc["camera"], 8)
    ctx = core.Context(0)
    live = core.DeviceScene(flat, ctx=ctx)
    side = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)]
    create, host, stream_host, stream_dev = [], [], [], []
    made = []

    def make():
        made.append(core.DeviceScene(flat, ctx=ctx))

    n_q = 64
    for rep in range(REPS + 1):  # repetition 0 is the warm-up
        c = _wall(make)
        made.pop().close()
        k = rep % len(views)
        h = _wall(lambda: live.set_camera(views[k]))
        torch.cuda.synchronize()
        s = _wall(lambda: live.set_camera(views[(k + 1) % len(views)], stream=side.cuda_stream))
        side.synchronize()
        ev[0].record(side)
        for q in range(n_q):
            live.set_camera(views[q % len(views)], stream=side.cuda_stream)
        ev[1].record(side)
        side.synchronize()
        if rep:
            create.append(c); host.append(h); stream_host.append(s); stream_dev.append(ev[0].elapsed_time(ev[1]) / n_q)
    n_prims = int(len(flat.prim_kind))
    live.close()
    ctx.close()
    return {"scene": which, "primitives": n_prims, "create": _median_ms(create), "set_camera_host_form": _median_ms(host),
            "set_camera_stream_form_host_time": _median_ms(stream_host), "set_camera_stream_form_device_time_per_call": _median_ms(stream_dev)}


def _slow_path():
    """the moving cover scene: every set_camera rebuilds (disjoint shutters), against creating the scene"""
    from raytrace_clj_amd import camera as cam, core, flatten as fl
    sc = _scene("C2m")
    flat = fl.flatten(sc)
    c0 = sc["camera"]
    early = cam.ThinLensCamera(c0.origin, c0.lleft, c0.horiz, c0.vert, c0.u, c0.v, c0.w, c0.aperture, 0.0, 0.4)
    late = cam.ThinLensCamera(c0.origin, c0.lleft, c0.horiz, c0.vert, c0.u, c0.v, c0.w, c0.aperture, 0.6, 1.0)
    ctx = core.Context(0)
    live = core.DeviceScene(_with_camera(flat, early), ctx=ctx)
    create, rebuild = [], []
    made = []
    for rep in range(REPS + 1):
        c = _wall(lambda: made.append(core.DeviceScene(flat, ctx=ctx)))
        made.pop().close()
        flags = []
        r = _wall(lambda: flags.append(live.set_camera(late if rep % 2 == 0 else early)))
        assert flags == [True], "the disjoint shutter must rebuild"
        if rep:
            create.append(c); rebuild.append(r)
    n_prims = int(len(flat.prim_kind))
    live.close()
    ctx.close()
    return {"scene": "C2m", "primitives": n_prims, "create": _median_ms(create), "set_camera_rebuild": _median_ms(rebuild)}


def step_set_camera():
    return {"fast_path": [_fast_path("C3"), _fast_path("CB")], "slow_path": _slow_path()}


def step_orbit():
    import torch
    from raytrace_clj_amd import camera as cam, core, dist, flatten as fl
    nx, ny, ns = 800, 400, 64
    sc = _scene("C2")
    flat = fl.flatten(sc)
    views = cam.orbit(sc["camera"], VIEWS, [0.0, 0.0, 0.0])
    flats = [_with_camera(flat, v) for v in views]
    ctx = core.Context(0)
    live = core.DeviceScene(flat, ctx=ctx)
    out = torch.zeros((ny, nx, 3), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    fp = dist.FramePipeline(flat, nx, ny, 0, 1, 0, depth=2)

    def recreate():
        for f in flats:
            ds = core.DeviceScene(f, ctx=ctx)
            ds.render_device(nx, ny, ns, out)
            torch.cuda.synchronize()
            ds.close()

    def host_form():
        for v in views:
            live.set_camera(v)
            live.render_device(nx, ny, ns, out)
            torch.cuda.synchronize()

    def render_views():
        live.render_views(views, nx, ny, ns)

    def pipeline():
        for v in views:
            fp.step(ns, camera=v)
        fp.sync()

    variants = [("recreate_and_render", recreate), ("set_camera_and_render", host_form), ("render_views_one_sync", render_views),
                ("frame_pipeline_depth_2", pipeline)]
    times = {name: [] for name, _ in variants}
    for rep in range(REPS + 1):
        order = variants if rep % 2 == 0 else variants[::-1]
        for name, fn in order:
            t = _wall(fn) / VIEWS
            if rep:
                times[name].append(t)
    fp.close()
    live.close()
    ctx.close()
    return {"scene": "C2", "nx": nx, "ny": ny, "ns": ns, "views": VIEWS, "per_view": {name: _median_ms(t) for name, t in times.items()}}


def child(step, out_dir):
    res = step_set_camera() if step == "set-camera" else step_orbit()
    with open(os.path.join(out_dir, step + ".json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "camera"))
    ap.add_argument("--child")
    ap.add_argument("steps", nargs="*")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        child(a.child, a.out)
        return 0
    for step in a.steps or list(STEPS):
        if step not in STEPS:
            raise SystemExit("unknown step %r; one of %s" % (step, ", ".join(STEPS)))
        print("== %s (limit %d s)" % (step, STEPS[step]), flush=True)
        try:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step, "--out", a.out], check=True, timeout=STEPS[step], cwd=ROOT)
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
            print("step %s failed: %s -- stopping, nothing else is started" % (step, e), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
