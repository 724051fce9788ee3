"""Adaptive sampling on the GPU, measured: what it buys and what it costs when it buys nothing.

    python scripts/gpu_adaptive.py [--out DIR] [step ...]      steps: buys-C3 buys-FINAL cost-C3 kernels denoised (default: all, in this order)

Every step is a child process of its own under a time limit; the first one that fails (or runs out of time) ends the run, nothing is started after
it.  Each step writes DIR/<step>.json.  Times are device events on one stream around the whole sequence of calls of a variant, after a warm-up,
median of 5, with the compared variants alternated in the same process.

  buys-C3     1920x1080, 10 001 spheres, first 64, chunk 64, cap 256: for eps at the 25 % / 50 % / 75 % quantiles of the frame's own per-tile noise
              after the first round, the share of pixel-samples traced and the time against the one-shot render at the cap
  buys-FINAL  make-final 500x500, first 32, chunk 32, cap 128: the same
  cost-C3     C3 as 4 x 64 with eps = 0 (no tile retires: checked) against refine 4 x 64, the progressive path; the progressive run is
              measured twice per repetition, the difference of its two medians is its own spread
  kernels     rocprofv3 --kernel-trace --stats over one adaptive C3 run: time per call of the three adaptive kernels
  denoised    adaptive sampling steered by the denoised frame's noise estimate, two children: (1) C3: one
              rtmi_adaptive_retire_device call (kernel + compaction + synchronise) next to the adaptive round it follows; then the Cornell box
              600x600 and C3, first 64, chunk 64, cap 256, eps = the median per-tile maximum of the first round's filtered noise: time and
              pixel-samples of render_adaptive -> denoise -> adaptive_retire against uniform-at-cap + denoise and against the raw criterion
              at the same eps; (2) rocprofv3 --kernel-trace --stats over one such C3 run, in a run of its own: adaptive_retire_kernel's line"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEPS = {"buys-C3": 420, "buys-FINAL": 300, "cost-C3": 300, "kernels": 300, "denoised": 540}  # step -> time limit in seconds
REPS = 5


def _scene(which):
    import raytrace_clj_amd as r
    if which == "C3":
        nx, ny = 1920, 1080
        return r.scene.make_random_scene(nx, ny, 50, False, mix=(0.8, 0.95)), nx, ny, 64, 64, 256
    if which == "CB":
        nx, ny = 600, 600
        return r.scene.make_cornell_box(nx, ny), nx, ny, 64, 64, 256
    nx, ny = 500, 500
    return r.scene.make_final(nx, ny), nx, ny, 32, 32, 128


class Bench:
    def __init__(self, which):
        import torch
        from raytrace_clj_amd import core
        self.torch, self.core = torch, core
        sc, self.nx, self.ny, self.first, self.chunk, self.cap = _scene(which)
        self.ctx = core.Context(0)
        self.ds = core.DeviceScene(sc, ctx=self.ctx)
        nx, ny = self.nx, self.ny
        self.lin = torch.zeros((ny, nx, 3), dtype=torch.float64, device="cuda")
        self.q = torch.zeros((ny, nx, 3), dtype=torch.uint8, device="cuda")
        self.err = torch.zeros((ny, nx), dtype=torch.float64, device="cuda")
        self.spp = torch.zeros((ny, nx), dtype=torch.int32, device="cuda")
        self.cnt = torch.zeros(2, dtype=torch.int64, device="cuda")
        # A stream of torch's own, handed to every call: stream 0 would mean "the context's stream" to the library, which is a non-blocking
        # stream and not ordered with the null stream the events would be recorded on (dist.py, "Streams").
        torch.cuda.synchronize()  # the buffers are zeroed on torch's default stream
        self.side = torch.cuda.Stream()
        self.stream = self.side.cuda_stream
        assert self.stream != 0

    def rounds(self):
        k = 0
        while k < self.cap:
            n = min(self.first if k == 0 else self.chunk, self.cap - k)
            yield k, n
            k += n

    def one_shot(self):
        self.ds.render_device(self.nx, self.ny, self.cap, self.lin, self.q, self.cnt, stream=self.stream)

    def progressive(self):
        for k, n in self.rounds():
            self.ds.render_progressive_device(self.nx, self.ny, k, n, self.lin, self.q, self.err, self.cnt, stream=self.stream)

    def adaptive(self, eps):
        for k, n in self.rounds():
            self.ds.render_adaptive_device(self.nx, self.ny, k, n, eps, self.lin, self.q, self.err, self.spp, self.cnt, stream=self.stream)
            if self.ctx.adaptive_status()[0] == 0:
                break

    def filter_buffers(self):
        """the buffers of the adaptive-denoised loop: the features (rendered here, once) and the filtered frame"""
        t, nx, ny = self.torch, self.nx, self.ny
        with t.cuda.stream(self.side):
            self.ft = t.zeros((ny, nx, 8), dtype=t.float64, device="cuda")
            self.flin = t.zeros((ny, nx, 3), dtype=t.float64, device="cuda")
            self.fq = t.zeros((ny, nx, 3), dtype=t.uint8, device="cuda")
            self.ferr = t.zeros((ny, nx), dtype=t.float64, device="cuda")
        self.ds.render_features_device(nx, ny, self.core.FEATURE_SAMPLES, self.ft, None, stream=self.stream)
        self.side.synchronize()

    def denoise(self):
        self.ctx.denoise_device(self.nx, self.ny, self.lin, self.err, self.ft, self.flin, self.fq, self.ferr, stream=self.stream)

    def uniform_denoised(self):
        """uniform at the cap with its noise estimate, then the filter: the existing path"""
        self.ds.render_progressive_device(self.nx, self.ny, 0, self.cap, self.lin, self.q, self.err, self.cnt, stream=self.stream)
        self.denoise()

    def adaptive_then_denoise(self, eps):
        """the raw criterion, the frame filtered once at the end"""
        self.adaptive(eps)
        self.denoise()

    def adaptive_denoised(self, eps):
        """one stream, no host copy: render_adaptive (raw rule at eps 0) -> denoise -> adaptive_retire on the filtered noise plane"""
        for k, n in self.rounds():
            self.ds.render_adaptive_device(self.nx, self.ny, k, n, 0.0, self.lin, self.q, self.err, self.spp, self.cnt, stream=self.stream)
            self.denoise()
            self.ctx.adaptive_retire_device(self.nx, self.ny, self.ferr, eps, stream=self.stream)
            if self.ctx.adaptive_status()[0] == 0:
                break

    def first_round_filtered_tile_noise(self):
        """per-tile maxima of the filtered noise plane after the first round of a uniform frame"""
        import numpy as np
        self.ds.render_progressive_device(self.nx, self.ny, 0, self.first, self.lin, None, self.err, None, stream=self.stream)
        self.denoise()
        self.side.synchronize()
        e = self.ferr.cpu().numpy()
        ty, tx = (self.ny + 7) // 8, (self.nx + 7) // 8
        pad = np.full((ty * 8, tx * 8), -np.inf)
        pad[:self.ny, :self.nx] = e
        return pad.reshape(ty, 8, tx, 8).max(axis=(1, 3)).ravel()

    def timed(self, fn):
        t = self.torch
        e0, e1 = t.cuda.Event(enable_timing=True), t.cuda.Event(enable_timing=True)
        with t.cuda.stream(self.side):  # events and work on the one stream
            e0.record(self.side)
            fn()
            e1.record(self.side)
        self.side.synchronize()
        return e0.elapsed_time(e1)

    def alternate(self, variants):
        """{name: fn} -> {name: [ms] * REPS}, one warm-up of each first"""
        for fn in variants.values():
            self.timed(fn)
        ms = {name: [] for name in variants}
        for _ in range(REPS):
            for name, fn in variants.items():
                ms[name].append(self.timed(fn))
        return ms

    def first_round_tile_noise(self):
        """per-tile maxima of out_stderr after the first round of a uniform frame"""
        import numpy as np
        self.ds.render_progressive_device(self.nx, self.ny, 0, self.first, None, None, self.err, None, stream=self.stream)
        self.side.synchronize()
        e = self.err.cpu().numpy()
        ty, tx = (self.ny + 7) // 8, (self.nx + 7) // 8
        pad = np.full((ty * 8, tx * 8), -np.inf)
        pad[:self.ny, :self.nx] = e
        return pad.reshape(ty, 8, tx, 8).max(axis=(1, 3)).ravel()

    def close(self):
        self.ctx.progressive_release()
        self.ds.close()
        self.ctx.close()


def _summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "ms": ms}


def step_buys(which):
    import numpy as np
    b = Bench(which)
    try:
        noise = b.first_round_tile_noise()
        out = {"scene": which, "nx": b.nx, "ny": b.ny, "first": b.first, "chunk": b.chunk, "cap": b.cap, "tiles": int(noise.size), "runs": []}
        for quantile in (0.25, 0.5, 0.75):
            eps = float(np.quantile(noise[np.isfinite(noise)], quantile))
            ms = b.alternate({"one_shot": b.one_shot, "adaptive": lambda: b.adaptive(eps)})
            active, total, pixel_samples = b.ctx.adaptive_status()
            levels, counts = np.unique(b.spp.cpu().numpy(), return_counts=True)
            out["runs"].append({"eps": eps, "quantile": quantile, "one_shot": _summary(ms["one_shot"]), "adaptive": _summary(ms["adaptive"]),
                                "share_of_pixel_samples": pixel_samples / (b.nx * b.ny * b.cap), "tiles_active_at_end": active,
                                "k_at_end": b.ctx.progressive_samples(), "pixels_per_level": dict(zip(map(int, levels), map(int, counts)))})
        return out
    finally:
        b.close()


def step_cost():
    b = Bench("C3")
    try:
        ms = b.alternate({"progressive": b.progressive, "adaptive_eps0": lambda: b.adaptive(0.0), "progressive_again": b.progressive})
        b.adaptive(0.0)
        b.side.synchronize()
        active, total, pixel_samples = b.ctx.adaptive_status()
        assert active == total and pixel_samples == b.nx * b.ny * b.cap, "a tile retired at eps = 0: this scene is no zero-gain case"
        p, a, p2 = (statistics.median(ms[n]) for n in ("progressive", "adaptive_eps0", "progressive_again"))
        spread = abs(p - p2)
        base = min(p, p2)
        allowed = base + spread + 0.01 * base  # the progressive run, its own spread, 1 %
        return {"scene": "C3", "rounds": "4 x 64", "tiles": total, "tiles_active_at_end": active, "progressive": _summary(ms["progressive"]),
                "adaptive_eps0": _summary(ms["adaptive_eps0"]), "progressive_again": _summary(ms["progressive_again"]),
                "progressive_spread_ms": spread, "allowed_ms": allowed, "over_progressive": a / base - 1.0, "within_allowance": a <= allowed}
    finally:
        b.close()


def step_retire_cost():
    """C3: the first adaptive round (64 samples, the raw rule at eps 0) and the rtmi_adaptive_retire_device call that follows it, on a filtered
    noise plane computed once; every repetition starts a new frame, so the retire call does the same work each time"""
    import numpy as np
    b = Bench("C3")
    try:
        b.filter_buffers()
        noise = b.first_round_filtered_tile_noise()
        eps = float(np.quantile(noise[np.isfinite(noise)], 0.5))
        t = b.torch
        rounds, retires, retired = [], [], []
        for rep in range(REPS + 1):  # the first repetition is the warm-up
            ev = [t.cuda.Event(enable_timing=True) for _ in range(3)]
            with t.cuda.stream(b.side):
                ev[0].record(b.side)
                b.ds.render_adaptive_device(b.nx, b.ny, 0, b.first, 0.0, b.lin, b.q, b.err, b.spp, b.cnt, stream=b.stream)
                ev[1].record(b.side)
                n = b.ctx.adaptive_retire_device(b.nx, b.ny, b.ferr, eps, stream=b.stream)
                ev[2].record(b.side)
            b.side.synchronize()
            if rep:
                rounds.append(ev[0].elapsed_time(ev[1]))
                retires.append(ev[1].elapsed_time(ev[2]))
                retired.append(n)
        return {"scene": "C3", "eps": eps, "tiles": int(noise.size), "tiles_retired_per_call": retired, "adaptive_round_64spp": _summary(rounds),
                "retire_call": _summary(retires)}
    finally:
        b.close()


def step_denoised_buys(which):
    import numpy as np
    b = Bench(which)
    try:
        b.filter_buffers()
        noise = b.first_round_filtered_tile_noise()
        eps = float(np.quantile(noise[np.isfinite(noise)], 0.5))
        samples = {}

        def run(name, fn):
            def go():
                fn()
                samples[name] = b.ctx.adaptive_status()
            return go

        ms = b.alternate({"uniform_cap_denoise": run("uniform_cap_denoise", b.uniform_denoised),
                          "adaptive_raw_then_denoise": run("adaptive_raw_then_denoise", lambda: b.adaptive_then_denoise(eps)),
                          "adaptive_denoised": run("adaptive_denoised", lambda: b.adaptive_denoised(eps))})
        full = b.nx * b.ny * b.cap
        out = {"scene": which, "nx": b.nx, "ny": b.ny, "first": b.first, "chunk": b.chunk, "cap": b.cap, "eps": eps, "tiles": int(noise.size)}
        for name in ms:
            active, total, pixel_samples = samples[name]
            out[name] = dict(_summary(ms[name]), share_of_pixel_samples=pixel_samples / full, tiles_active_at_end=active)
        return out
    finally:
        b.close()


def step_denoised_profiled_run():
    """what `denoised` runs under rocprofv3: one warm-up and one adaptive-denoised C3 run at the median eps"""
    import numpy as np
    b = Bench("C3")
    try:
        b.filter_buffers()
        noise = b.first_round_filtered_tile_noise()
        eps = float(np.quantile(noise[np.isfinite(noise)], 0.5))
        for _ in range(2):
            b.adaptive_denoised(eps)
        b.side.synchronize()
    finally:
        b.close()


def step_profiled_run():
    """what `kernels` runs under rocprofv3: one warm-up and one adaptive C3 run at the median eps"""
    import numpy as np
    b = Bench("C3")
    try:
        noise = b.first_round_tile_noise()
        eps = float(np.quantile(noise[np.isfinite(noise)], 0.5))
        for _ in range(2):
            b.adaptive(eps)
        b.side.synchronize()
    finally:
        b.close()


def step_kernels(out_dir, limit, child_step="profiled-run", sub="kernel_trace", keep=("adaptive_", "frame_", "trace_kernel")):
    d = os.path.join(out_dir, sub)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", "adaptive", "--output-format", "csv", "--", "timeout", "-k", "10", str(max(30, limit - 30)), sys.executable, os.path.abspath(__file__),
           "--child", child_step, "--out", out_dir]
    subprocess.run(cmd, check=True, timeout=limit, cwd=ROOT)
    rows = []
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        for row in csv.DictReader(open(path)):
            name = row.get("Name") or row.get("KernelName") or ""
            if any(k in name for k in keep):
                rows.append({"kernel": name.split("(")[0][:120], "calls": int(row["Calls"]), "total_ms": float(row["TotalDurationNs"]) * 1e-6,
                             "average_ms": float(row["AverageNs"]) * 1e-6})
    assert rows, "no kernel statistics found under %s" % d
    return {"scene": "C3", "runs": 2, "kernels": rows}


def child(step, out_dir):
    if step == "profiled-run":
        step_profiled_run()
        return
    if step == "denoised-profiled-run":
        step_denoised_profiled_run()
        return
    if step == "denoised":
        res = {"retire_cost": step_retire_cost(), "buys": [step_denoised_buys("CB"), step_denoised_buys("C3")]}
    else:
        res = step_buys(step.split("-")[1]) if step.startswith("buys-") else step_cost()
    with open(os.path.join(out_dir, step + ".json"), "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "out", "adaptive"))
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
            if step == "kernels":
                res = step_kernels(a.out, STEPS[step])
                with open(os.path.join(a.out, "kernels.json"), "w") as f:
                    json.dump(res, f, indent=1)
                print(json.dumps(res))
            else:
                subprocess.run([sys.executable, os.path.abspath(__file__), "--child", step, "--out", a.out], check=True, timeout=STEPS[step], cwd=ROOT)
                if step == "denoised":  # the new kernel's line, from a profiled run of its own
                    res = step_kernels(a.out, 300, "denoised-profiled-run", "kernel_trace_denoised", ("adaptive_", "frame_", "denoise_", "trace_kernel"))
                    with open(os.path.join(a.out, "denoised_kernels.json"), "w") as f:
                        json.dump(res, f, indent=1)
                    print(json.dumps(res))
        except (subprocess.CalledProcessError, subprocess.TimeoutExpired, AssertionError) as e:
            print("step %s failed: %s -- stopping, nothing else is started" % (step, e), flush=True)
            return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
