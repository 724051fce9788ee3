"""Editing the materials of a live scene on the GPU, measured: what rtmi_scene_set_materials* costs next to destroying
the scene and creating it anew with the same arrays -- the only way there was before.

    python scripts/gpu_materials.py [--out DIR]

The measurement is one child process under a time limit; it writes DIR/materials.json.  At C3 (1920x1080's scene: 10 001 spheres) and at the
Cornell box, a warm-up and the median of 5 repetitions, the variants alternated inside every repetition; wall clock around host calls (the
stream is idle when the clock starts and synchronised before it stops), device events around work that is only queued:

  recreate           close() + DeviceScene(edited): flattening is outside the clock
  in_place           set_materials(edited), the host form: one material's colour and one material's parameter change
  in_place_all       the host form with every Constant colour of the scene changed (whole tables travel either way)
  stream_host_time   set_materials(edited, stream=), host time per call: pack, compare with the mirror, launch the changed rows
  stream_device_time the same, device time per call: events around 64 queued calls (each alternates between two edits, so rows travel)
  rebuild            set_materials on its slow path: the edit alternately appends a material and takes it away again"""
import argparse
import copy
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

LIMIT = 420  # seconds
REPS = 5
TABLES = ("mat_kind", "mat_tex", "mat_param", "tex_kind", "tex_param", "tex_child", "prim_mat")


def _median_ms(samples):
    return {"median_ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples), "n": len(samples)}


def _wall(fn):
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def _scene(which):
    import raytrace_clj_amd as r
    return r.scene.make_random_scene(1920, 1080, 50, False) if which == "C3" else r.scene.make_cornell_box(600, 600)


def _edit(flat, change):
    import numpy as np
    f = copy.copy(flat)
    for name in TABLES:
        setattr(f, name, np.array(getattr(flat, name)))
    change(f)
    return f


def _edits(flat):
    """two small edits to alternate between, one that touches every Constant, and one that appends a material"""
    import numpy as np
    from raytrace_clj_amd import flatten as fl
    lamb = int(np.flatnonzero(flat.mat_kind == fl.MAT_LAMBERTIAN)[-1])
    other = int(np.flatnonzero(flat.mat_kind != fl.MAT_DIELECTRIC)[0])

    def small(shade):
        def change(f):
            f.tex_param[f.mat_tex[lamb], 0:3] = shade
            f.mat_param[other] = 0.25 * shade[0]
        return change

    def every(mix):
        def change(f):
            const = f.tex_kind == fl.TEX_CONSTANT
            f.tex_param[const, 0:3] = mix * f.tex_param[const, 0:3] + 0.05
        return change

    def grow(f):
        f.mat_kind = np.append(f.mat_kind, fl.MAT_METAL).astype(np.int32)
        f.mat_tex = np.append(f.mat_tex, f.mat_tex[lamb]).astype(np.int32)
        f.mat_param = np.append(f.mat_param, 0.1)
        f.prim_mat[int(np.flatnonzero(f.prim_mat == lamb)[0])] = len(f.mat_kind) - 1
    return [_edit(flat, small((0.2, 0.5, 0.8))), _edit(flat, small((0.7, 0.3, 0.1)))], [_edit(flat, every(0.9)), _edit(flat, every(0.8))], _edit(flat, grow)


def measure(which):
    import torch
    from raytrace_clj_amd import core, flatten as fl
    flat = fl.flatten(_scene(which))
    small, every, grown = _edits(flat)
    ctx = core.Context(0)
    live = core.DeviceScene(flat, ctx=ctx)
    side = torch.cuda.Stream()
    ev = [torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)]
    names = ("recreate", "in_place", "in_place_all", "stream_host_time", "stream_device_time", "rebuild")
    times = {n: [] for n in names}
    spare = [core.DeviceScene(flat, ctx=ctx)]
    n_q = 64

    def recreate(f):
        spare.pop().close()
        spare.append(core.DeviceScene(f, ctx=ctx))

    for rep in range(REPS + 1):  # repetition 0 is the warm-up
        a, b = small[rep % 2], small[1 - rep % 2]
        t = {}
        t["recreate"] = _wall(lambda: recreate(a))
        flags = []
        t["in_place"] = _wall(lambda: flags.append(live.set_materials(a)))
        t["in_place_all"] = _wall(lambda: flags.append(live.set_materials(every[rep % 2])))
        assert live.set_materials(a) is False  # (outside the clock: the stream form is for a few rows, its starting point must be near)
        torch.cuda.synchronize()
        t["stream_host_time"] = _wall(lambda: flags.append(live.set_materials(b, stream=side.cuda_stream)))
        side.synchronize()
        ev[0].record(side)
        for q in range(n_q):
            live.set_materials(small[q % 2], stream=side.cuda_stream)
        ev[1].record(side)
        side.synchronize()
        t["stream_device_time"] = ev[0].elapsed_time(ev[1]) / n_q
        assert flags == [False, False, False], "the edits must fit"
        t["rebuild"] = _wall(lambda: flags.append(live.set_materials(grown)))
        assert flags[-1] is True, "another material count must rebuild"
        assert live.set_materials(flat) is True  # back to the scene's own count (outside the clock)
        if rep:
            for n in names:
                times[n].append(t[n])
    res = {"scene": which, "primitives": int(len(flat.prim_kind)), "materials": int(len(flat.mat_kind)), "textures": int(len(flat.tex_kind)),
           "stream_calls_per_device_sample": n_q}
    res.update({n: _median_ms(v) for n, v in times.items()})
    spare.pop().close()
    live.close()
    ctx.close()
    return res


def child(out_dir):
    res = {"scenes": [measure("C3"), measure("CB")]}
    with open(os.path.join(out_dir, "materials.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "materials"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        child(a.out)
        return 0
    print("== materials (limit %d s)" % LIMIT, flush=True)
    try:
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--out", a.out], check=True, timeout=LIMIT, cwd=ROOT)
    except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
        print("the measurement failed: %s" % e, flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
