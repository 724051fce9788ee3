"""Light-sampled frames on several devices, measured: what the record pass, the gather and the assemble add to a chunk, and
what the adaptive loop costs through the frame object.

    python scripts/gpu_multi_lit.py [--out DIR] [--only chunk|loop]

One child process per measurement, each under its own time limit; the first failure ends the run.  Every child writes DIR/multi_lit_<name>.json.  A
warm-up, then the median of 5 with minimum - maximum, the variants alternated in one process; scripts/gpu_nee.py's scenes.

  chunk   1920 x 1080, mis, depth 50, ONE chunk of 4 samples into a fresh frame with every tile listed:
            (a) rtmi_render_lit_tiles_device on one context (device events around the call on a stream of its own, and the wall time of the call
                with its synchronisation);
            (b) rtmi_multi_lit_render_device with one replica (wall time: the call returns with every stream synchronised, and its launches lie on
                the contexts' own streams, where a caller cannot place events);
            (c) the same with replicas [0, 0]: the control flow of two replicas on one device, NOT a scaling figure.
          (b) / (a) on the wall times is what the record pass and the assemble add to a chunk.  The frames of (a), (b) and (c) are compared bit for bit.
  loop    the Cornell box 512 x 512, mis, first 16, chunk 16, cap 256 (scripts/gpu_lit_tiles.py's loop and its eps ladder), wall time of the whole loop
          with its last download: (a) DeviceScene.refine_lit_adaptive (buffers resident across the rounds) against the same rounds through
          MultiDevice.lit_render_device + lit_retire with the outputs resident on replica 0's device, (b) one replica, (c) replicas [0, 0]; b_host is
          MultiDevice.refine_lit_adaptive with one replica, the host-array driver that brings the frame back every round.  The per-round imbalance of
          the two replicas -- the largest replica's listed tiles over the mean -- is printed: tiles are not re-dealt between rounds.

A curve over distinct devices cannot be taken on a one-GPU host."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.gpu_lit_tiles import EPS_LADDER, LOOP  # noqa: E402
from scripts.gpu_nee import DEPTH, LIMIT, PER_PIXEL, REPS, VIEW, _median, _scene  # noqa: E402

CHILDREN = ("chunk_cornell", "chunk_C3", "loop_cornell")


def measure_chunk(which):
    import torch

    from raytrace_clj_amd import core, dist
    nx, ny = VIEW
    sc = _scene(which, nx, ny)
    ctx = core.Context(0)
    ds = core.DeviceScene(sc, ctx=ctx)
    mds = {"b": dist.MultiDevice(sc, [0]), "c": dist.MultiDevice(sc, [0, 0])}
    n_tiles = dist.n_tiles(nx, ny)
    f64 = dict(dtype=torch.float64, device="cuda")
    one = dict(lin=torch.zeros((ny, nx, 3), **f64), err=torch.zeros((ny, nx), **f64), q=torch.zeros((ny, nx, 3), dtype=torch.uint8, device="cuda"),
               state=torch.zeros((nx * ny, 10), **f64), cnt=torch.zeros(4, dtype=torch.int64, device="cuda"),
               tiles=torch.arange(n_tiles, dtype=torch.int32, device="cuda"))
    out = {k: dict(lin=torch.zeros((ny, nx, 3), **f64), err=torch.zeros((ny, nx), **f64), q=torch.zeros((ny, nx, 3), dtype=torch.uint8, device="cuda"),
                   smp=torch.zeros((ny, nx), dtype=torch.int32, device="cuda"), cnt=torch.zeros(4, dtype=torch.int64, device="cuda")) for k in mds}
    side = torch.cuda.Stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    kw = dict(estimator="mis", depth=DEPTH)
    times = {"a_events": [], "a": [], "b": [], "c": [], "b_gather": [], "c_gather": []}
    torch.cuda.synchronize()
    for rep in range(REPS + 1):
        row = {}
        one["state"].zero_()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with torch.cuda.stream(side):
            e0.record()
            ds.render_lit_tiles_device(nx, ny, 0, PER_PIXEL, n_tiles, one["tiles"], one["lin"], one["err"], one["q"], state=one["state"],
                                       out_counters=one["cnt"], stream=side.cuda_stream, **kw)
            e1.record()
        side.synchronize()
        row["a"] = (time.perf_counter() - t0) * 1e3
        row["a_events"] = e0.elapsed_time(e1)
        for name, md in mds.items():
            md.lit_reset(nx, ny)
            o = out[name]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            md.lit_render_device(nx, ny, PER_PIXEL, o["lin"], o["q"], o["err"], o["smp"], o["cnt"], **kw)
            row[name] = (time.perf_counter() - t0) * 1e3
            row[name + "_gather"] = md.last_gather_ms()
        if rep:
            for k, v in row.items():
                times[k].append(v)
        print("rep %d: " % rep + ", ".join("%s %.3f ms" % kv for kv in sorted(row.items())), flush=True)
    torch.cuda.synchronize()
    res = {"scene": which, "view": list(VIEW), "per_pixel": PER_PIXEL, "depth": DEPTH, "tiles": n_tiles,
           "record_bytes_per_replica": {"b": (n_tiles * 320 + 4) * 8, "c": (-(-n_tiles // 2) * 320 + 4) * 8}}
    res.update({k: _median(v) for k, v in times.items()})
    res["b_over_a"] = res["b"]["median_ms"] / res["a"]["median_ms"]
    res["c_over_a"] = res["c"]["median_ms"] / res["a"]["median_ms"]
    res["gather_path"] = {k: md.last_gather_path() for k, md in mds.items()}
    res["ok"] = all(bool(torch.equal(one["lin"], o["lin"]) and torch.equal(one["q"], o["q"]) and torch.equal(one["cnt"], o["cnt"]))
                    and bool((o["smp"] == PER_PIXEL).all()) for o in out.values())  # the same frame
    for md in mds.values():
        md.close()
    ds.close()
    ctx.close()
    return res


def measure_loop(which):
    import numpy as np
    import torch

    from raytrace_clj_amd import core, dist
    nx, ny, first, chunk, cap = (LOOP[k] for k in ("nx", "ny", "first", "chunk", "cap"))
    sc = _scene(which, nx, ny)
    ctx = core.Context(0)
    ds = core.DeviceScene(sc, ctx=ctx)
    mds = {"b": dist.MultiDevice(sc, [0]), "c": dist.MultiDevice(sc, [0, 0])}
    kw = dict(estimator="mis", depth=DEPTH)

    def timed(f):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = f()
        torch.cuda.synchronize()
        return out, (time.perf_counter() - t0) * 1e3
    ds.refine_lit_adaptive(nx, ny, 2 * chunk, chunk, 1.0, first=first, **kw)  # warm-up
    for md in mds.values():
        md.refine_lit_adaptive(nx, ny, 2 * chunk, chunk, 1.0, first=first, **kw)
    chosen = None
    for eps in EPS_LADDER:
        out, ms = timed(lambda: ds.refine_lit_adaptive(nx, ny, cap, chunk, eps, first=first, **kw))
        share = float(out[3].sum()) / (nx * ny * cap)
        print("eps %g: %.1f %% of the pixel-samples, %.1f ms" % (eps, 100 * share, ms), flush=True)
        if 0.25 <= share <= 0.75:
            chosen = (eps, share)
            break
    res = {"scene": which, "loop": LOOP, "depth": DEPTH, "ok": chosen is not None}
    f64 = dict(dtype=torch.float64, device="cuda")
    held = dict(lin=torch.zeros((ny, nx, 3), **f64), q=torch.zeros((ny, nx, 3), dtype=torch.uint8, device="cuda"), err=torch.zeros((ny, nx), **f64),
                smp=torch.zeros((ny, nx), dtype=torch.int32, device="cuda"), cnt=torch.zeros(4, dtype=torch.int64, device="cuda"))

    def resident(md, eps):  # the loop with the outputs resident on replica 0's device: per round one render call, one retire call, the call's four counters and one integer back
        md.lit_reset(nx, ny)
        k, active, total = 0, dist.n_tiles(nx, ny), np.zeros(4, np.int64)
        while k < cap and active:
            n = min(first if k == 0 else chunk, cap - k)
            md.lit_render_device(nx, ny, n, held["lin"], held["q"], held["err"], held["smp"], held["cnt"], **kw)
            k += n
            total += held["cnt"].cpu().numpy()
            active = md.lit_retire(nx, ny, eps)
        return held["lin"].cpu().numpy(), held["q"].cpu().numpy(), held["err"].cpu().numpy(), held["smp"].cpu().numpy(), total.astype(np.uint64)
    if chosen:
        eps = chosen[0]
        for md in mds.values():
            resident(md, 1.0)  # warm-up
        runs, last = {"a": [], "b": [], "c": [], "b_host": []}, {}
        for rep in range(REPS):
            for name, f in (("a", lambda: ds.refine_lit_adaptive(nx, ny, cap, chunk, eps, first=first, **kw)),
                            ("b", lambda: resident(mds["b"], eps)), ("c", lambda: resident(mds["c"], eps)),
                            ("b_host", lambda: mds["b"].refine_lit_adaptive(nx, ny, cap, chunk, eps, first=first, **kw))):
                last[name], ms = timed(f)
                runs[name].append(ms)
            print("rep %d: " % rep + ", ".join("%s %.1f ms" % (k, v[-1]) for k, v in sorted(runs.items())), flush=True)
        last["c_host"] = mds["c"].refine_lit_adaptive(nx, ny, cap, chunk, eps, first=first, **kw)  # untimed: the round lists of two replicas
        same = all(np.array_equal(last["a"][i], last[k][i]) for k in ("b", "c", "b_host", "c_host") for i in range(5))
        same = same and all(len(last["a"][5]) == len(last[k][5]) and all(np.array_equal(x[1], y[1]) for x, y in zip(last["a"][5], last[k][5]))
                            for k in ("b_host", "c_host"))
        imbalance = []
        for k, tiles in last["c_host"][5]:
            per = [int((tiles % 2 == r).sum()) for r in range(2)]
            imbalance.append({"k": k, "listed": per, "max_over_mean": (max(per) / (sum(per) / 2.0)) if sum(per) else 1.0})
            print("round k=%d: replica lists %s, largest over mean %.3f" % (k, per, imbalance[-1]["max_over_mean"]), flush=True)
        res.update({"eps": eps, "share": chosen[1], "ms": {k: _median(v) for k, v in runs.items()}, "rounds": len(last["a"][5]),
                    "imbalance_two_replicas": imbalance, "ok": bool(same)})
        res["b_over_a"] = res["ms"]["b"]["median_ms"] / res["ms"]["a"]["median_ms"]
    for md in mds.values():
        md.close()
    ds.close()
    ctx.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "multi_lit"))
    ap.add_argument("--only", default=None, choices=("chunk", "loop"))
    ap.add_argument("--child", default=None, choices=CHILDREN)
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)
    if a.child:
        kind, which = a.child.split("_", 1)
        res = {"chunk": measure_chunk, "loop": measure_loop}[kind](which)
        with open(os.path.join(a.out, "multi_lit_%s.json" % a.child), "w") as f:
            json.dump(res, f, indent=1)
        print(json.dumps(res), flush=True)
        if not res["ok"]:
            print("the measurement did not meet its own condition (see \"ok\" in the code): the figures are not to be used", flush=True)
            return 1
        return 0
    for which in CHILDREN:
        if a.only and not which.startswith(a.only):
            continue
        print("== multi lit, %s (limit %d s)" % (which, LIMIT), flush=True)
        try:
            subprocess.run([sys.executable, os.path.abspath(__file__), "--child", which, "--out", a.out], check=True, timeout=LIMIT, cwd=ROOT)
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired) as e:
            print("the measurement failed: %s" % e, flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
