"""The entry grid's one-pass form (rtmi_device.h: bvh_grid_entry): the end of a piece of the walk is computed for every lane, the segment is
clipped to it and ONE rectangle of cells is taken.  Where a traversal starts must never change a result: on rays aimed at the places where the
clipped form decides differently from the two-rectangle form it replaced -- segment ends next to the two-cell bound, starts next to cell
borders, direction components at the float traversal's acceptance threshold, origins outside the grid, the layer and the scene bound -- the
hits must equal the exact flat scan's bit for bit, for several grid shapes, with and without the walk, in both precisions, and so must whole
renders and their counters; and the walk must still shorten traversals."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raytrace_clj_amd as r
from raytrace_clj_amd import core
from raytrace_clj_amd import flatten as fl

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from test_gpu_parity import grazing_rays, tangent_rays, random_rays, layer_scene  # noqa: E402

FLT_MAX = 3.4028234663852886e38
GRIDS = (1, 5, 23, 64)  # RTMI_GRID: cells per side (1: the library's own choice)
PER_FAMILY = 20000
SCENES = {"layer": lambda: layer_scene(3, n=1200), "cover11m": lambda: r.scene.make_random_scene(160, 80, 11, True)}


def grid_geometry(f):
    """the layer's box as scene_build.h takes it (every sphere but the ground and the few much taller than the median; a moving sphere's box
    spans its sweep) and the library's own number of cells per side -- to within the boxes' inflation, far below the 1/256 of a cell the
    rays are aimed with"""
    g = f.prim_geom
    keep = g[:, 3] < 50
    c0, c1, rad = g[keep, 0:3], g[keep, 4:7], g[keep, 3:4]
    lo, hi = np.minimum(c0, c1) - rad, np.maximum(c0, c1) + rad
    h = hi[:, 1] - lo[:, 1]
    layer = h <= 3.0 * np.sort(h)[len(h) // 2]
    lo, hi = lo[layer].min(0), hi[layer].max(0)
    ext = hi - lo
    auto = int(round(min(np.sqrt(layer.sum() / 3.5), min(ext[0], ext[2]) / (4.5 * ext[1]))))
    return lo, hi, max(2, min(auto, 256))


def ground_y(x, z):
    return np.sqrt(1000.0 ** 2 - x * x - z * z) - 1000.0  # both scenes stand on a sphere of radius 1000 around (0, -1000, 0)


def targeted_rays(f, n, seed):
    """five families of n rays, each spread over the grid shapes of GRIDS, both horizontal axes and both direction signs"""
    rng = np.random.default_rng(seed)
    lo, hi, auto = grid_geometry(f)
    top = hi[1]
    out = []
    shapes = [auto if G == 1 else G for G in GRIDS]
    k = n // len(shapes)
    for G in shapes:
        cs = np.array([(hi[0] - lo[0]) / G, (hi[2] - lo[2]) / G])
        org = np.array([lo[0], lo[2]])
        margin = 2.0 ** -16 * 2.0 * max(abs(lo).max(), abs(hi).max())  # ~ the rectangle's growth e for an origin inside the layer (world units)

        def world(cells):  # [k, 2] cell coordinates -> x, z
            return org + cells * cs

        # (1) the segment ends on the ground within +-2/256 of a cell of the bound of the two cells that hold its start, along `axis`; the
        # other axis travels up to 1.5 cells either way (sometimes it is the tighter one).  t-min = 0: the start is the origin itself
        axis = rng.integers(0, 2, k)
        sign = rng.choice([-1.0, 1.0], k)
        cell = np.stack([rng.integers(0, G, k), rng.integers(0, G, k)], axis=1).astype(np.float64)
        start = cell + rng.uniform(0.0, 1.0, (k, 2))
        end = start + rng.uniform(-1.5, 1.5, (k, 2))
        bound = np.where(sign > 0, cell[np.arange(k), axis] + 2.0, cell[np.arange(k), axis] - 1.0)
        end[np.arange(k), axis] = bound + rng.uniform(-2.0 / 256.0, 2.0 / 256.0, k)
        s, e = world(start), world(end)
        o = np.stack([s[:, 0], ground_y(s[:, 0], s[:, 1]) + rng.uniform(0.02, 0.9, k) * top, s[:, 1]], axis=1)
        p = np.stack([e[:, 0], ground_y(e[:, 0], e[:, 1]), e[:, 1]], axis=1)
        out.append(np.concatenate([o, (p - o) * rng.choice([1.0, 1e-3, 50.0], (k, 1))], axis=1))
        # (2) the start within the margin of a cell border (half of them moved back by t-min = 0.001 of the direction, so that the range starts
        # there for the default t-min too); short and long segments, every direction
        border = rng.integers(0, G + 1, (k, 2)).astype(np.float64)
        on = rng.random((k, 2)) < 0.7
        start = np.where(on, border, border + rng.uniform(0.0, 1.0, (k, 2)))
        s = world(start) + on * margin * rng.choice([0.0, 1e-9, -1e-9, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0], (k, 2))
        d = np.stack([rng.normal(0, 1, k), -np.abs(rng.normal(0, 1, k)) * rng.choice([1e-3, 0.03, 0.3], k), rng.normal(0, 1, k)], axis=1)
        d *= rng.choice([0.3, 1.0, 4.0], (k, 1)) * cs.min() * rng.choice([1.0, 1e-3, 50.0], (k, 1))
        o = np.stack([s[:, 0], ground_y(s[:, 0], s[:, 1]) + rng.uniform(0.02, 0.9, k) * top, s[:, 1]], axis=1)
        o -= np.where(rng.random((k, 1)) < 0.5, 0.001, 0.0) * d
        out.append(np.concatenate([o, d], axis=1))
        # (3) one direction component at 1e-12 of the largest and around it (below it the ray takes the exact flat scan, from it on the grid:
        # its 1 / d is then ~1e12 / dmax); long, nearly horizontal segments from inside the layer
        s = world(rng.uniform(0.0, G, (k, 2)))
        d = np.stack([rng.normal(0, 1, k), -np.abs(rng.normal(0, 1, k)) * rng.choice([1e-3, 0.03], k), rng.normal(0, 1, k)], axis=1)
        d *= rng.choice([1.0, 1e-3, 50.0], (k, 1))
        dmax = np.abs(d).max(1)
        which = rng.integers(0, 3, k)
        which = np.where(np.abs(d[np.arange(k), which]) == dmax, (which + 1) % 3, which)
        d[np.arange(k), which] = dmax * 1e-12 * rng.choice([0.5, 0.999, 0.99999994, 1.0, 1.0000001, 1.001, 2.0, 10.0], k) * rng.choice([-1.0, 1.0], k)
        o = np.stack([s[:, 0], ground_y(s[:, 0], s[:, 1]) + rng.uniform(0.02, 0.9, k) * top, s[:, 1]], axis=1)
        out.append(np.concatenate([o, d], axis=1))
        # (4) origins outside the grid's extent (beside it by a fraction of a cell up to many cells) and outside the layer's box (above it,
        # below the ground's top), aimed across the layer at grazing angles: the range starts where the ray enters the box
        side = rng.integers(0, 5, k)
        s = rng.uniform(-0.5, G + 0.5, (k, 2))
        off = rng.choice([1e-6, 0.01, 0.5, 3.0, 40.0], k)
        s[:, 0] = np.where(side == 0, -off, np.where(side == 1, G + off, s[:, 0]))
        s[:, 1] = np.where(side == 2, -off, np.where(side == 3, G + off, s[:, 1]))
        s = world(s)
        y = np.where(side == 4, top * (1.0 + rng.choice([1e-7, 0.01, 1.0, 30.0], k)), rng.uniform(-0.2, 1.2, k) * top)
        o = np.stack([s[:, 0], y, s[:, 1]], axis=1)
        t = world(rng.uniform(0.0, G, (k, 2)))
        p = np.stack([t[:, 0], rng.uniform(-0.3, 1.0, k) * top, t[:, 1]], axis=1)
        out.append(np.concatenate([o, (p - o) * rng.choice([1.0, 1e-3, 50.0], (k, 1))], axis=1))
        # (5) far origins: outside the scene bound by factors up to 1e6 (every box plane moves out by 2^-20 |o|), aimed at points of the layer
        t = world(rng.uniform(0.0, G, (k, 2)))
        p = np.stack([t[:, 0], rng.uniform(0.0, 1.0, k) * top, t[:, 1]], axis=1)
        w = np.stack([rng.normal(0, 1, k), np.abs(rng.normal(0, 1, k)) * rng.choice([1e-3, 0.03, 0.5], k), rng.normal(0, 1, k)], axis=1)
        w /= np.linalg.norm(w, axis=1, keepdims=True)
        o = p + w * rng.choice([1.2e3, 1e4, 1e5, 1e6], (k, 1)) * rng.uniform(1.0, 3.0, (k, 1))
        out.append(np.concatenate([o, (p - o) * rng.choice([1.0, 1e-3, 2.0], (k, 1))], axis=1))
    rays = np.concatenate(out)
    return np.concatenate([rays, rng.random((len(rays), 1))], axis=1)


_CASES = {}


def case(name):
    """the scene, its probe rays and the flat scan's answers: computed once, shared by every test, never changed"""
    if name not in _CASES:
        flat = fl.flatten(SCENES[name]())
        rays = np.concatenate([targeted_rays(flat, PER_FAMILY, 21), grazing_rays(flat, 20000, 11), tangent_rays(flat, 10000, 12), random_rays(5000, 13, spread=40.0)])
        ctx = core.Context(0)
        ctx.set_option("accel", 0)
        ds = core.DeviceScene(flat, ctx=ctx)
        ref = {}
        for prec in ("f64", "f32"):
            ref[prec] = (ds.probe_hit(rays, precision=prec), ds.probe_hit(rays, 0.0, FLT_MAX, precision=prec), ds.render(160, 80, 8, precision=prec))
            for a in ref[prec][:2]:
                a.setflags(write=False)
        ds.close(); ctx.close()
        _CASES[name] = (flat, rays, ref)
    return _CASES[name]


def test_probe_rays_reach_the_layer():
    """the targeted families are about segments inside the layer: most of them must hit something (the ground at least), in every family"""
    for name in SCENES:
        flat, rays, ref = case(name)
        hit = ref["f64"][1][:, 0] == 1
        n = PER_FAMILY // len(GRIDS)
        for G in range(len(GRIDS)):
            for fam in range(5):
                part = hit[(G * 5 + fam) * n:(G * 5 + fam + 1) * n]
                assert part.mean() > 0.3, (name, GRIDS[G], fam, part.mean())


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_grid_entry_equals_the_flat_scan(name, grid, monkeypatch):
    flat, rays, ref = case(name)
    monkeypatch.setenv("RTMI_GRID", str(grid))
    monkeypatch.setenv("RTMI_GRID_KMAX", "4")
    for walk in ("1", "0"):
        monkeypatch.setenv("RTMI_GRID_WALK", walk)
        ctx = core.Context(0)
        ds = core.DeviceScene(flat, ctx=ctx)  # the grid is built with the scene
        try:
            for prec in ("f64", "f32"):
                a = ds.probe_hit(rays, precision=prec)  # t-min = 0.001
                b = ds.probe_hit(rays, 0.0, FLT_MAX, precision=prec)
                assert np.array_equal(a, ref[prec][0]), (name, grid, walk, prec, "t-min 0.001", int((a != ref[prec][0]).any(axis=1).sum()))
                assert np.array_equal(b, ref[prec][1]), (name, grid, walk, prec, "t-min 0", int((b != ref[prec][1]).any(axis=1).sum()))
                for lanes in (12, 0):
                    ctx.set_option("suspend_lanes", lanes)
                    out = ds.render(160, 80, 8, precision=prec)
                    for x, y in zip(out, ref[prec][2]):  # linear frame, 8-bit frame, counters
                        assert np.array_equal(x, y), (name, grid, walk, prec, lanes)
        finally:
            ds.close(); ctx.close()


@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_walk_is_still_taken(name, monkeypatch):
    """node visits per segment with the walk stay below 0.97 x those without it, in the same build: a clipped form that sent its pieces to the root
    of the whole tree (a rectangle that no longer fits) would still be right, and would lose exactly this"""
    flat, rays, ref = case(name)
    monkeypatch.setenv("RTMI_GRID", "1")
    monkeypatch.setenv("RTMI_GRID_KMAX", "4")
    visits = {}
    for walk in ("1", "0"):
        monkeypatch.setenv("RTMI_GRID_WALK", walk)
        ctx = core.Context(0)
        ds = core.DeviceScene(flat, ctx=ctx)
        try:
            assert ds.tree_info()[2] > 0, (name, "the scene must get a grid")
            ctx.set_option("count_traversal", 1)
            out = ds.render(160, 80, 8)
            visits[walk] = ctx.last_traversal_counters()[0] / 2 / float(out[2][0])
        finally:
            ds.close(); ctx.close()
    print(name, "node visits per segment: walk %.4f, no walk %.4f" % (visits["1"], visits["0"]))
    assert visits["1"] < 0.97 * visits["0"], (name, visits)
