#!/usr/bin/env python3
"""Temporal accumulation evaluated on the CPU: the oracle's frames and features and the numpy restatement of the tests
(tests/reproject_reference.py), no device.

    python scripts/eval_reproject.py [--truth 1024] [--trials 4] [--views 6] [cornell] [cover]

Pinhole views of the classic Cornell box at 96x96 and of the small cover scene at 200x100, turned about the vertical axis through the look-at
point by 1 and by 3 degrees per view, 4 spp per view, a new seed per view.  The last view's accumulated frame is compared with a frame of
--truth samples from another seed: RMS error relative to the raw 4-spp frame of that view, averaged over --trials sets of seeds (one trial is
too noisy: the Cornell light makes heavy tails).  A grid over sigma_d, sigma_n, sigma_a (0 = test off) and max_history; per point one JSON line.
Then, per scene and step, the best point, the chosen defaults (core.REPROJECT_*), and a uniform frame of the same total samples.
With --views 16 --caps-only the caps separate (6 views of 4 spp never reach 32): the default sigmas only, every cap."""
import argparse
import copy
import itertools
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import denoise_reference as dr             # noqa: E402
import frame_reference as fr               # noqa: E402
import reproject_reference as rr           # noqa: E402
import raytrace_clj_amd as r               # noqa: E402
from oracle.oracle import Oracle           # noqa: E402
from oracle.tree import attach_tree        # noqa: E402
from raytrace_clj_amd import core          # noqa: E402
from raytrace_clj_amd import flatten as fl  # noqa: E402
from raytrace_clj_amd.util import vec3      # noqa: E402

NS, NA = 4, core.FEATURE_SAMPLES
SIGMA_D = (0.0, 0.02, 0.05, 0.1)
SIGMA_N = (0.0, 0.25, 0.5)
SIGMA_A = (0.0, 0.1, 0.2)
CAPS = (8.0, 16.0, 32.0, float("inf"))
DEFAULTS = (core.REPROJECT_SIGMA_D, core.REPROJECT_SIGMA_N, core.REPROJECT_SIGMA_A, core.REPROJECT_MAX_HISTORY)


def scene(which):
    """-> (world, nx, ny, lookfrom, lookat, vfov)"""
    if which == "cornell":
        nx = ny = 96
        return r.scene.make_cornell_box(nx, ny)["world"], nx, ny, np.array([278.0, 278.0, -800.0]), np.array([278.0, 278.0, 278.0]), 40
    nx, ny = 200, 100
    return r.scene.make_random_scene(nx, ny, 3, False)["world"], nx, ny, np.array([13.0, 2.0, 3.0]), np.array([0.0, 0.0, 0.0]), 20


def flat_view(world, nx, ny, lookfrom, lookat, vfov, degrees):
    a = np.radians(degrees)
    d = lookfrom - lookat
    frm = lookat + np.array([d[0] * np.cos(a) + d[2] * np.sin(a), d[1], -d[0] * np.sin(a) + d[2] * np.cos(a)])
    cam = r.camera.pinhole_camera(lookfrom=vec3(*frm), lookat=vec3(*lookat), vup=vec3(0, 1, 0), vfov=vfov, aspect=nx / ny)
    return attach_tree(fl.flatten({"camera": cam, "world": world}), world)


def evaluate(which, step, views, trials, truth_spp, threads, sigmas=None):
    o = Oracle("f64")
    world, nx, ny, lookfrom, lookat, vfov = scene(which)
    flats = [flat_view(world, nx, ny, lookfrom, lookat, vfov, step * k) for k in range(views)]
    truth = o.render(flats[-1], nx, ny, truth_spp, fr.DEPTH, fr.SEED + 999983, nthreads=threads)[0]
    sets = []
    for t in range(trials):
        seeds = [fr.SEED + 1000 * (t + 1) + k for k in range(views)]
        sets.append([(np.asarray(f.cam, np.float64), o.render(f, nx, ny, NS, fr.DEPTH, s, nthreads=threads)[0], None,
                      dr.feature_frame(dr.feature_samples(o, f, nx, ny, NA, seed=s))) for f, s in zip(flats, seeds)])
    raw = float(np.mean([rr.rms(v[-1][1], truth) for v in sets]))
    uniform = float(np.mean([rr.rms(o.render(flats[-1], nx, ny, NS * views, fr.DEPTH, fr.SEED + 5000 + t, nthreads=threads)[0], truth)
                             for t in range(trials)]))
    base = {"scene": which, "degrees_per_view": step, "views": views, "spp_per_view": NS, "trials": trials, "truth_spp": truth_spp}
    print(json.dumps(dict(base, rms_raw=raw, rms_uniform_same_total=uniform, ratio_uniform=uniform / raw)), flush=True)
    rows = {}
    caps = CAPS if NS * views > min(CAPS) else (float("inf"),)
    points = itertools.product(SIGMA_D, SIGMA_N, SIGMA_A, caps) if sigmas is None else [tuple(sigmas) + (cap,) for cap in caps] + [(0.0, 0.0, 0.0, float("inf"))]
    for sd, sn, sa, cap in points:
        if cap != float("inf") and cap >= NS * views:
            continue  # such a cap never binds: the same frame as no cap
        res = [rr.accumulate(v, NS, cap, sd, sn, sa)[-1] for v in sets]
        ratio = float(np.mean([rr.rms(x[0], truth) for x in res])) / raw
        rows[sd, sn, sa, cap] = ratio
        print(json.dumps(dict(base, sigma_d=sd, sigma_n=sn, sigma_a=sa, max_history=cap, ratio=ratio,
                              share_with_history=float(np.mean([x[4] for x in res])), mean_weight=float(np.mean([x[2].mean() for x in res])))), flush=True)
    best = min(rows, key=rows.get)
    d = DEFAULTS if DEFAULTS in rows else DEFAULTS[:3] + (float("inf"),)
    print(json.dumps(dict(base, best=dict(zip(("sigma_d", "sigma_n", "sigma_a", "max_history"), best)), ratio_best=rows[best],
                          defaults=dict(zip(("sigma_d", "sigma_n", "sigma_a", "max_history"), d)), ratio_defaults=rows[d],
                          ratio_no_tests=rows[0.0, 0.0, 0.0, float("inf")], ratio_uniform=uniform / raw)), flush=True)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--truth", type=int, default=1024)
    ap.add_argument("--trials", type=int, default=4)
    ap.add_argument("--views", type=int, default=6)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--caps-only", action="store_true", help="the default sigmas only, every cap (for --views beyond 6)")
    ap.add_argument("scenes", nargs="*", default=["cornell", "cover"])
    a = ap.parse_args()
    total = {}
    for which in a.scenes:
        for step in (1.0, 3.0):
            for k, v in evaluate(which, step, a.views, a.trials, a.truth, a.threads, DEFAULTS[:3] if a.caps_only else None).items():
                total.setdefault(k, []).append(v)
    mean = {k: float(np.mean(v)) for k, v in total.items()}
    order = sorted(mean, key=mean.get)
    print(json.dumps({"mean_ratio_over_scenes_and_steps": [dict(zip(("sigma_d", "sigma_n", "sigma_a", "max_history", "ratio"), k + (mean[k],)))
                                                           for k in order[:8]]}))


if __name__ == "__main__":
    main()
