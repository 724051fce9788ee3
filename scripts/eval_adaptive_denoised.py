#!/usr/bin/env python3
"""Adaptive sampling steered by the denoised frame's noise estimate, evaluated on the CPU: the oracle's individual
samples and the numpy restatements of the tests (tests/adaptive_denoised_reference.py), no device.

    python scripts/eval_adaptive_denoised.py [--truth 1024] [cornell] [cover]

Pinhole views of the classic Cornell box at 96x96 and of the small cover scene at 200x100, first 16, chunk 16, cap 64, the library's default
filter, eps in {0.02, 0.04, 0.08}, against a frame of --truth samples from another seed.  Per eps one JSON line: the share of pixel-samples
taken; the RMS error of the final filtered frame; the same for a uniform frame at the same mean spp, filtered; the same for adaptive sampling on
the RAW criterion at the same eps, filtered once at the end; and where the filtered estimate is low but the error is not: over the tiles the
filtered criterion retired, the RMS error of their filtered pixels, and the tiles whose own RMS error exceeds 2 eps."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import adaptive_denoised_reference as adr  # noqa: E402
import adaptive_reference as ar            # noqa: E402
import denoise_reference as dr             # noqa: E402
import frame_reference as fr               # noqa: E402
import raytrace_clj_amd as r               # noqa: E402
from oracle.oracle import Oracle           # noqa: E402
from oracle.tree import attach_tree        # noqa: E402
from raytrace_clj_amd import flatten as fl  # noqa: E402
from raytrace_clj_amd.util import vec3      # noqa: E402

FIRST, CHUNK, CAP = 16, 16, 64
EPS = (0.02, 0.04, 0.08)


def scene(which):
    if which == "cornell":
        nx = ny = 96
        world = r.scene.make_cornell_box(nx, ny)["world"]
        cam = r.camera.pinhole_camera(lookfrom=vec3(278, 278, -800), lookat=vec3(278, 278, 0), vup=vec3(0, 1, 0), vfov=40, aspect=nx / ny)
    else:
        nx, ny = 200, 100
        world = r.scene.make_random_scene(nx, ny, 3, False)["world"]
        cam = r.camera.pinhole_camera(lookfrom=vec3(13, 2, 3), lookat=vec3(0, 0, 0), vup=vec3(0, 1, 0), vfov=20, aspect=nx / ny)
    return attach_tree(fl.flatten({"camera": cam, "world": world}), world), nx, ny


def tile_rms(img, truth):
    """RMS error per 8x8 tile over its pixels inside the image -> [tiles_y, tiles_x]"""
    ny, nx = img.shape[:2]
    tx, ty = fr.tiles_of(nx, ny)
    sq, n = np.zeros((ty * 8, tx * 8)), np.zeros((ty * 8, tx * 8))
    sq[:ny, :nx] = ((img - truth) ** 2).mean(axis=2)
    n[:ny, :nx] = 1.0
    return np.sqrt(sq.reshape(ty, 8, tx, 8).sum(axis=(1, 3)) / n.reshape(ty, 8, tx, 8).sum(axis=(1, 3)))


def evaluate(which, truth_spp):
    o = Oracle("f64")
    flat, nx, ny = scene(which)
    smp, _ = fr.frame_samples(o, flat, nx, ny, CAP)
    feat = dr.feature_frame(dr.feature_samples(o, flat, nx, ny, adr.NA))
    truth = o.render(flat, nx, ny, truth_spp, fr.DEPTH, fr.SEED + 1, nthreads=16)[0]
    m2 = ar.welford_m2(smp, list(range(2, CAP + 1)))
    frame_of = lambda n_px: ar.expected_frame(smp, n_px)
    stderr_of = lambda k: ar.stderr_plane(m2[k], k)
    filtered = lambda n_px: dr.denoise(frame_of(n_px), ar.compose(stderr_of, n_px), feat, **adr.FILTER)
    full = nx * ny * CAP
    for k in (FIRST, CAP):
        flt, _, ferr = filtered(np.full((ny, nx), k))
        print(json.dumps({"scene": which, "uniform_spp": k, "rms_raw": dr.rms(frame_of(np.full((ny, nx), k)), truth), "rms_filtered": dr.rms(flt, truth),
                          "median_tile_max_raw_stderr": float(np.median(ar.tile_max(stderr_of(k)))),
                          "median_tile_max_filtered_stderr": float(np.median(ar.tile_max(ferr)))}), flush=True)
    for eps in EPS:
        rounds = adr.schedule(frame_of, stderr_of, feat, nx, ny, FIRST, CHUNK, CAP, eps)
        last = rounds[-1]
        n_px = ar.per_pixel(last["n_t"], nx, ny)
        mean = n_px.sum() / (nx * ny)
        same = max(2, int(round(mean)))
        raw = ar.schedule(stderr_of, nx, ny, FIRST, CHUNK, CAP, eps)[-1]
        raw_px = ar.per_pixel(raw[1], nx, ny)
        retired = ~last["active"]
        per_tile = tile_rms(last["flt_linear"], truth)
        sel = ar.per_pixel(retired, nx, ny)
        print(json.dumps({
            "scene": which, "eps": eps, "rounds": [int(m["active"].sum()) for m in rounds], "tiles": int(last["active"].size),
            "share_of_pixel_samples": float(n_px.sum() / full), "mean_spp": float(mean), "rms_filtered": dr.rms(last["flt_linear"], truth),
            "uniform_same_mean_spp": same, "rms_uniform_same_mean_filtered": dr.rms(filtered(np.full((ny, nx), same))[0], truth),
            "raw_share_of_pixel_samples": float(raw_px.sum() / full), "raw_tiles_active_at_cap": int(raw[2].sum()),
            "rms_raw_criterion_filtered": dr.rms(filtered(raw_px)[0], truth),
            "retired_tiles": int(retired.sum()),
            "rms_of_retired_tiles_pixels": dr.rms(last["flt_linear"][sel], truth[sel]) if sel.any() else None,
            "retired_tiles_with_rms_above_2_eps": int((per_tile[retired] > 2 * eps).sum()),
            "worst_retired_tile_rms": float(per_tile[retired].max()) if retired.any() else None}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--truth", type=int, default=1024)
    ap.add_argument("scenes", nargs="*")
    a = ap.parse_args()
    for which in a.scenes or ["cornell", "cover"]:
        if which not in ("cornell", "cover"):
            raise SystemExit("unknown scene %r; one of cornell, cover" % which)
        evaluate(which, a.truth)
    return 0


if __name__ == "__main__":
    sys.exit(main())
