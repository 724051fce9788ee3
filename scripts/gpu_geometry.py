"""Moving the primitives of a live scene on the GPU, measured: what rtmi_scene_set_geometry costs next to destroying the
scene and creating it anew with the same arrays -- the only way there was before -- and what a displaced primitive costs a frame.

    python scripts/gpu_geometry.py [--out DIR]

The measurement is one child process under a time limit; it writes DIR/geometry.json.  At C3 (1920x1080's scene: 10 001 spheres) and at the
Cornell box, a warm-up and the median of 5 repetitions, the variants alternated inside every repetition; wall clock around host calls (the
device is idle when the clock starts and synchronised before it stops, so the queued refit is inside), device events around the refit itself:

  recreate            close() + DeviceScene(edited): flattening is outside the clock
  in_place            set_geometry(edited): a few spheres shrunk and nudged, nothing displaced
  in_place_displaced  set_geometry(edited): one sphere, already displaced, dragged on (C3 only: the Cornell box has no entry grid)
  rebuild             set_geometry(edited, mode="rebuild")
  in_place_first      the first in-place edit after a build: it also makes the refit plan (the node array read back, heights, two device tables)
  refit               device time of the refit launches of the in_place edit (rtmi_scene_last_refit_ms), and their number
  frame_displaced_k   C3 only: the frame (1920x1080, 8 samples, by the library's events) with k = 0, 1, 4 and 14 - n_big spheres displaced ...
  frame_rebuilt_k     ... and of the same scene after mode="rebuild" (everything home again)"""
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

LIMIT = 540  # seconds
REPS = 5
FRAME = (1920, 1080, 8)


def _median_ms(samples):
    return {"median_ms": statistics.median(samples), "min_ms": min(samples), "max_ms": max(samples), "n": len(samples)}


def _wall(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def _scene(which):
    import raytrace_clj_amd as r
    return r.scene.make_random_scene(1920, 1080, 50, False) if which == "C3" else r.scene.make_cornell_box(600, 600)


def _edit(flat, change):
    import numpy as np
    f = copy.copy(flat)
    f.prim_geom = np.array(flat.prim_geom, np.float64)
    f.xform_param = np.array(flat.xform_param, np.float64).reshape(-1, 3)
    change(f.prim_geom, f.xform_param)
    return f


def _small(flat):
    import numpy as np
    from raytrace_clj_amd import flatten as fl
    k = np.asarray(flat.prim_kind) & ~fl.PRIM_BOUNDARY
    return np.flatnonzero((k <= fl.PRIM_MOVING) & (np.abs(flat.prim_geom[:, 3]) < 0.5))


def _edits(flat, which):
    """two in-place edits to alternate between"""
    import numpy as np
    from raytrace_clj_amd import flatten as fl
    if which == "C3":
        pick = _small(flat)[::1000]

        def nudge(factor):
            def change(g, xp):
                g[pick, 3] *= factor
                g[pick, 0] += 1e-3
            return change
        return [_edit(flat, nudge(0.9)), _edit(flat, nudge(0.8))]
    tr = int(np.flatnonzero(flat.xform_kind == fl.XFORM_TRANSLATE)[-1])
    return [_edit(flat, lambda g, xp: xp.__setitem__((tr, 0), xp[tr, 0] + 10.0)), _edit(flat, lambda g, xp: xp.__setitem__((tr, 0), xp[tr, 0] - 10.0))]


def _carried(flat, which, lift=1.0, shift=0.0):
    def change(g, xp):
        for i in which:
            g[i, 0], g[i, 2] = -g[i, 0] * 0.5 + shift, -g[i, 2] * 0.5
            g[i, 1] += lift
    return _edit(flat, change)


def measure(which):
    import torch
    from raytrace_clj_amd import core, flatten as fl
    flat = fl.flatten(_scene(which))
    pair = _edits(flat, which)
    ctx = core.Context(0, timing=True)
    live = core.DeviceScene(flat, ctx=ctx)
    dragged = core.DeviceScene(flat, ctx=ctx) if which == "C3" else None
    spare = [core.DeviceScene(flat, ctx=ctx)]
    sync = torch.cuda.synchronize
    rebuilt = core.DeviceScene(flat, ctx=ctx)
    names = ["recreate", "in_place", "rebuild", "in_place_first", "refit"] + (["in_place_displaced"] if dragged else [])
    times = {n: [] for n in names}
    launches, records, displaced = set(), set(), set()
    small = _small(flat)
    if dragged:
        drag = [_carried(flat, small[:1], shift=0.0), _carried(flat, small[:1], shift=0.4)]
        assert dragged.set_geometry(drag[0])["displaced"] == 1

    def recreate(f):
        spare.pop().close()
        spare.append(core.DeviceScene(f, ctx=ctx))

    for rep in range(REPS + 1):  # repetition 0 is the warm-up
        a = pair[rep % 2]
        t, infos = {}, []
        t["recreate"] = _wall(lambda: recreate(a), sync)
        t["in_place"] = _wall(lambda: infos.append(live.set_geometry(a)), sync)
        assert infos[-1]["rebuilt"] is False and infos[-1]["displaced"] == 0, "the edit must fit"
        t["refit"] = live.last_refit_ms() if infos[-1]["launches"] else 0.0
        launches.add(infos[-1]["launches"])
        records.add(infos[-1]["nodes_refit"])
        if dragged:
            t["in_place_displaced"] = _wall(lambda: infos.append(dragged.set_geometry(drag[1 - rep % 2])), sync)
            assert infos[-1]["rebuilt"] is False and infos[-1]["displaced"] == 1
        t["rebuild"] = _wall(lambda: infos.append(rebuilt.set_geometry(a, mode="rebuild")), sync)
        assert infos[-1]["rebuilt"] is True
        t["in_place_first"] = _wall(lambda: infos.append(rebuilt.set_geometry(pair[1 - rep % 2])), sync)
        assert infos[-1]["rebuilt"] is False
        if rep:
            for n in names:
                times[n].append(t[n])
    res = {"scene": which, "primitives": int(len(flat.prim_kind)), "node_records": sorted(records), "refit_launches": sorted(launches), "tree_info": list(live.tree_info())}
    res.update({n: _median_ms(v) for n, v in times.items()})
    if dragged:  # the price of the big list per displaced primitive: the same frame with k spheres displaced, and after a rebuild
        nx, ny, ns = FRAME
        n_big = live.tree_info()[3]
        counts = [0, 1, 4, 14 - n_big]
        scenes, frames = {}, {}
        for k in counts:
            f = _carried(flat, small[:k]) if k else flat
            scenes[("displaced", k)] = core.DeviceScene(flat, ctx=ctx)
            assert scenes[("displaced", k)].set_geometry(f)["displaced"] == k
            scenes[("rebuilt", k)] = core.DeviceScene(flat, ctx=ctx)
            assert scenes[("rebuilt", k)].set_geometry(f, mode="rebuild")["rebuilt"] is True
        for rep in range(REPS + 1):
            for key, ds in scenes.items():
                ds.render(nx, ny, ns)
                if rep:
                    frames.setdefault(key, []).append(ctx.last_trace_ms()[0])
        for (what, k), v in frames.items():
            res["frame_%s_%d" % (what, k)] = _median_ms(v)
        res["frame"] = {"nx": nx, "ny": ny, "ns": ns, "n_big": int(n_big)}
        for ds in scenes.values():
            ds.close()
        dragged.close()
    spare.pop().close()
    rebuilt.close()
    live.close()
    ctx.close()
    return res


def child(out_dir):
    res = {"scenes": [measure("C3"), measure("CB")]}
    with open(os.path.join(out_dir, "geometry.json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "geometry"))
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        child(a.out)
        return 0
    print("== geometry (limit %d s)" % LIMIT, flush=True)
    try:
        subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--out", a.out], check=True, timeout=LIMIT, cwd=ROOT)
    except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
        print("the measurement failed: %s" % e, flush=True)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
