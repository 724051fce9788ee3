"""CPU tests of the tree builder on deep, degenerate and threshold-sized input (host code only: rtmi_test_build_tree needs no device).  The
recipes of tests/tree_scenes.py are what tests/test_gpu_deep_trees.py renders; here the builder must give each of them the tree the table
says -- on the calling thread and on the team, with equal hashes -- and never a tree as deep as the traversal stack."""
import ctypes

import numpy as np
import pytest

from raytrace_clj_amd import _ffi
from tests import tree_scenes as ts

RTMI_E_ARG, RTMI_E_STATE = -1, -5


def _cam(at=ts.CAMERA_AT):
    c = np.zeros(24, np.float64)
    c[:3] = at
    return c


def _build(geom, threads, cam=None):
    L = _ffi.lib()
    geom = np.ascontiguousarray(geom, np.float64)
    cam = _cam() if cam is None else cam
    h, info, ms = np.zeros(1, np.uint64), np.zeros(4, np.int32), np.zeros(1)
    assert L.rtmi_test_build_tree(len(geom), _ffi.ptr(geom), _ffi.ptr(cam), threads, _ffi.ptr(h), _ffi.ptr(info), _ffi.ptr(ms)) == 0
    return int(h[0]), tuple(int(v) for v in info)


def test_getter_is_declared_bound_and_exported():
    assert "rtmi_scene_tree_info" in _ffi.SYMBOLS
    L = _ffi.lib()
    assert L.rtmi_version() >= 212
    info = np.full(4, 7, np.int32)
    assert L.rtmi_scene_tree_info(None, _ffi.ptr(info)) == RTMI_E_STATE and "scene" in L.rtmi_last_error().decode()
    assert L.rtmi_scene_tree_info(None, None) == RTMI_E_STATE
    assert (info == 7).all()  # a failing call writes nothing


@pytest.mark.parametrize("name", sorted(ts.HOST_TABLE))
def test_recipe_builds_the_tree_of_the_table(name):
    """one thread and the team: the same node array (hash) and the table's (node records, depth, grid cells, big primitives)"""
    geom = ts.sphere_geom(ts.build(name))
    out = [_build(geom, threads) for threads in (1, 8, 1, 8)]
    assert len(set(out)) == 1, out
    info = out[0][1]
    print(name, info)
    assert info[1] < ts.STACK - 1, "a tree this deep is one the traversal stack cannot hold: %r" % (info,)
    assert info == ts.HOST_TABLE[name]


def test_deepest_tree_is_the_builders_maximum():
    """the depth budget: SAH only where median splits can still finish below it -- RTMI_BVH_STACK - 3 = 29 is reached, never passed"""
    deepest = max(v[1] for v in ts.HOST_TABLE.values())
    assert deepest == ts.STACK - 3
    for n, q in ((2000, 0.9), (1500, 0.97), (400, 0.5), (300, 0.25)):
        cx, rad = ts.chain_geom(n, q, 0.15)
        geom = np.stack([cx, np.zeros(n), np.zeros(n), rad], axis=1)
        _, info = _build(np.concatenate([[[0.0, 0.0, 0.0, 60.0]], geom]), 1)
        print(n, q, info)
        assert info[0] == n - 1 and info[1] <= ts.STACK - 3  # (a tree the "cannot happen" fallback emptied would report 0 node records)


def test_the_dome_makes_the_tree_independent_of_the_camera():
    """the device tests look along the chain from CHAIN_CAMERA_AT: under the radius-60 dome the scene's bound, and with it the tree, is the same"""
    geom = ts.sphere_geom(ts.chain(1000, 0.9, 0.15))
    assert _build(geom, 1) == _build(geom, 1, _cam(ts.CHAIN_CAMERA_AT))


def test_chooser_thresholds_sit_where_the_recipes_straddle_them():
    assert ts.HOST_TABLE["cloud(128)"][0] == 127 and ts.HOST_TABLE["cloud(129)"][0] == 128   # time-slicing from 128 inner nodes on
    assert ts.HOST_TABLE["layer(255)"][2] == 0 and ts.HOST_TABLE["layer(256)"][2] > 0        # the entry grid from 256 layer primitives on
    assert ts.HOST_TABLE["many_big(20, 300)"][3] == 16                                       # the cap on big primitives
    # without the cap's four the tree over the 300 small spheres has 299 inner nodes: the other four shells are in it
    assert ts.HOST_TABLE["many_big(20, 300)"][0] == 299 + 4
    # twenty spheres of one size, each as large as the scene: sixteen stay out, four build a tree
    geom = ts.scene_sized(20)
    assert _build(geom, 1)[1][3] == 16 and _build(geom, 1)[1][0] == 3


def test_mixed_recipes_have_the_sizes_the_small_world_scan_switches_at():
    from raytrace_clj_amd import flatten as fl
    for n in (64, 65):
        assert fl.flatten(ts.scene(ts.mixed(n))).n_prims == n


def test_unboundable_spheres_are_kept_out_of_the_tree_and_the_build_returns():
    """non-finite coordinates and coordinates beyond 1e15 cannot be bounded: such spheres join the big primitives (exact test for every ray) while
    there is room, and the build still returns a tree over the rest"""
    base = ts.sphere_geom(ts.cloud(40, dome=False))
    odd = ts.UNBOUNDABLE
    for k in range(len(odd)):
        (_, one), (_, team) = _build(np.concatenate([base, odd[k:k + 1]]), 1), _build(np.concatenate([base, odd[k:k + 1]]), 8)
        assert one == team and one[3] == 1 and one[0] == 39 and one[1] < ts.STACK - 1, (odd[k], one)
    _, info = _build(np.concatenate([odd, base, odd, odd]), 1)  # 27 of them: sixteen big, eleven in the tree with boxes of +-1e15
    assert info[3] == 16 and info[0] == 40 + 11 - 1 and info[1] < ts.STACK - 1, info


def test_chain_rays_are_what_the_recipe_says():
    n, q, rho = 1000, 0.9, 0.15
    rays, n_fb = ts.chain_rays(n, q, rho, 19700, 41)
    assert len(rays) == 20000 and n_fb == 300
    main, fb = rays[:-n_fb], rays[-n_fb:]
    assert (np.abs(main[:, 3:6]) > 0.02).all()          # oblique: no component of a direction near zero
    assert (fb[:, 4] == 0).all()                        # the fallback rays: d.y = 0
    plus = main[:, 3] > 0
    assert abs(plus.mean() - 0.5) < 0.01 and (main[plus, 0] < 0).all()   # half travel towards +x and start beyond the small end
    assert np.array_equal(rays, ts.chain_rays(n, q, rho, 19700, 41)[0])  # seeded
