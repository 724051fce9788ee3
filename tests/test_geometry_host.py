"""CPU tests of the live scene's geometry (rtmi_scene_set_geometry): the C-ABI declares, binds and exports it, the argument errors answer
without a device and before the handle is examined, the Python hosts reject another structure before they touch the library, the edit's packer
produces the bytes creation's does (rtmi_test_pack_geometry), and the refit -- the host reference of refit_kernel's rule, rtmi_test_refit -- is
(a) the builder's own array when nothing moves, (b) an independent numpy bottom-up recomputation when something does, (c) silent about child
codes and roots.  The fit and displacement rules are exercised through the same hook, one case on each side of every condition."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import raytrace_clj_amd as r
from raytrace_clj_amd import _ffi, core, dist
from raytrace_clj_amd import flatten as fl
import geometry_cases as gc
import tree_scenes as ts
from test_clj_conformance import GPU_CLJ, check_calls, header_prototypes, is_list, map_values, read_forms, walk
from test_materials_host import SCENES

RTMI_E_ARG, RTMI_E_UNSUPPORTED, RTMI_E_STATE = -1, -3, -5
NAMES = ("rtmi_scene_set_geometry", "rtmi_test_pack_geometry", "rtmi_test_refit", "rtmi_test_refit_half", "rtmi_test_scene_nodes")


def test_prototypes_parse_and_are_bound():
    protos = header_prototypes()
    assert protos["rtmi_scene_set_geometry"] == ["handle", "i32", "double[]", "i32", "double[]", "i32", "int[]"]
    assert len(protos["rtmi_test_pack_geometry"]) == len(protos["rtmi_scene_create_ex"])  # creation's arrays, a flag and one output for ctx and out_scene
    assert set(NAMES) <= set(_ffi.SYMBOLS) and set(NAMES) <= set(protos)


def test_library_exports_the_symbols():
    assert os.path.exists(_ffi.LIB_PATH), "build with `make -C raytrace_clj_amd/csrc` or __graft_entry__.build()"
    L = ctypes.CDLL(_ffi.LIB_PATH)
    for name in NAMES:
        assert hasattr(L, name), name
    assert L.rtmi_version() >= 214


def test_argument_errors_answer_without_a_device_and_before_the_handle():
    L = _ffi.lib()
    err = lambda: L.rtmi_last_error().decode()
    p = _ffi.ptr
    info = np.full(4, 7, np.int32)
    g, xp = np.zeros((3, 9)), np.zeros((2, 3))
    assert L.rtmi_scene_set_geometry(None, 3, None, 2, p(xp), 0, p(info)) == RTMI_E_ARG and "NULL" in err()
    assert L.rtmi_scene_set_geometry(None, -1, p(g), 2, p(xp), 0, p(info)) == RTMI_E_ARG and "negative" in err()
    assert L.rtmi_scene_set_geometry(None, 3, p(g), -2, p(xp), 0, p(info)) == RTMI_E_ARG and "negative" in err()
    assert L.rtmi_scene_set_geometry(None, 3, p(g), 2, p(xp), 2, p(info)) == RTMI_E_ARG and "mode" in err()
    # good arguments (xform_param may be NULL: it stays): now the handle is what is reported
    assert L.rtmi_scene_set_geometry(None, 3, p(g), 2, p(xp), 0, p(info)) == RTMI_E_STATE and "scene" in err()
    assert L.rtmi_scene_set_geometry(None, 3, p(g), 2, None, 1, None) == RTMI_E_STATE and "scene" in err()
    n = np.zeros(1, np.int64)
    assert L.rtmi_test_scene_nodes(None, None, 0, None) == RTMI_E_ARG
    assert L.rtmi_test_scene_nodes(None, None, 0, n.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))) == RTMI_E_STATE
    assert list(info) == [7, 7, 7, 7]  # a failing call writes nothing


class _Handle:
    """a DeviceScene that never met the library: any call through its handle would fail loudly"""
    def __init__(self, flat):
        self.flat, self.handle, self.ctx = flat, None, None

    _geometry_arrays = core.DeviceScene._geometry_arrays


def test_set_geometry_rejects_another_structure_without_touching_the_library(monkeypatch):
    flat = fl.flatten(r.scene.make_cornell_box(36, 20))
    monkeypatch.setattr(_ffi, "lib", lambda: pytest.fail("the library was called"))
    ds = _Handle(flat)
    import copy

    def other(change):
        f = copy.copy(flat)
        for name in ("prim_kind", "prim_flip", "prim_xform", "xform_kind", "xform_param", "prim_geom"):
            setattr(f, name, np.array(getattr(flat, name)))
        change(f)
        return f

    box = int(np.flatnonzero(flat.prim_xform[:, 1] > 0)[0])
    cases = {
        "count": fl.flatten(r.scene.make_two_spheres(36, 20)),
        "kind": other(lambda f: f.prim_kind.__setitem__(0, fl.PRIM_TRIANGLE)),
        "flip": other(lambda f: f.prim_flip.__setitem__(0, 1 - f.prim_flip[0])),
        "chain": other(lambda f: f.prim_xform.__setitem__((box, 1), f.prim_xform[box, 1] - 1)),
        "xform kind": other(lambda f: f.xform_kind.__setitem__(0, fl.XFORM_ROTATE_Y if f.xform_kind[0] == fl.XFORM_TRANSLATE else fl.XFORM_TRANSLATE)),
        "xform count": other(lambda f: (setattr(f, "xform_kind", f.xform_kind[:-1]), setattr(f, "xform_param", f.xform_param[:-1]))),
    }
    for name, f in cases.items():
        with pytest.raises(ValueError):
            core.DeviceScene.set_geometry(ds, f)
        assert ds.flat is flat, name
    with pytest.raises(ValueError):
        core.DeviceScene.set_geometry(ds, flat, mode="sometimes")


def test_python_hosts_expose_the_edit():
    assert list(inspect.signature(core.DeviceScene.set_geometry).parameters) == ["self", "scene_or_flat", "mode"]
    assert inspect.signature(core.DeviceScene.set_geometry).parameters["mode"].default == "auto"
    assert list(inspect.signature(dist.MultiDevice.set_geometry).parameters) == ["self", "scene_or_flat", "mode"]
    step = inspect.signature(core.TemporalAccumulator.step).parameters
    assert step["geometry"].default is None and step["materials"].default is None
    assert "geometry" in core.TemporalAccumulator.step.__doc__ and "history" in core.TemporalAccumulator.step.__doc__


def test_gpu_clj_set_geometry_conforms_to_the_header():
    forms = read_forms(open(GPU_CLJ).read())
    by_name = {f[2]: f for f in forms if isinstance(f, list) and len(f) > 2 and f[1] in ("defn", "defn-")}
    assert "set-geometry" in by_name
    flat = [f for f in forms if is_list(f, "defn") and f[2] == "flatten-scene"][0]
    maps = [f for f in walk(flat) if isinstance(f, list) and f[0] == "{" and any(x == ":prim-kind" for x in f[1:])]
    protos, flat_map = header_prototypes(), map_values(maps[0])
    calls = {x[2].strip('"') for x in walk(by_name["set-geometry"]) if is_list(x, "call-int")}
    assert calls == {"rtmi_scene_set_geometry"}
    assert check_calls([by_name["set-geometry"]], protos, flat_map, True, "gpu.clj") == 1


# ---- one packer: the edit's geometry tables are creation's --------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SCENES))
def test_the_edit_packs_what_creation_packs(name):
    flat = fl.flatten(SCENES[name]())
    (rc0, h0), (rc1, h1) = gc.pack_geometry_hash(flat, 0), gc.pack_geometry_hash(flat, 1)
    assert (rc0, rc1) == (0, 0), _ffi.lib().rtmi_last_error().decode()
    assert h0 == h1


def test_the_geometry_hash_sees_every_kind_of_edit():
    seen = set()

    def both(f):
        (rc0, h0), (rc1, h1) = gc.pack_geometry_hash(f, 0), gc.pack_geometry_hash(f, 1)
        assert (rc0, rc1) == (0, 0) and h0 == h1 and h0 not in seen
        seen.add(h0)

    cover = fl.flatten(SCENES["cover-moving"]())
    both(cover)
    moving = int(np.flatnonzero(gc.kinds(cover) == fl.PRIM_MOVING)[0])
    static = int(gc.small_spheres(cover)[0])
    both(gc.edited(cover, lambda g, xp: g.__setitem__((static, 0), g[static, 0] + 0.25)))       # a centre
    both(gc.edited(cover, lambda g, xp: g.__setitem__((static, 3), g[static, 3] * 0.5)))        # a radius (r*r of the records, the cull entry)
    both(gc.edited(cover, lambda g, xp: g.__setitem__((moving, 5), g[moving, 5] + 0.125)))      # a MovingSphere's center1
    box = fl.flatten(SCENES["cornell"]())
    both(box)
    tr = int(np.flatnonzero(box.xform_kind == fl.XFORM_TRANSLATE)[0])
    ro = int(np.flatnonzero(box.xform_kind == fl.XFORM_ROTATE_Y)[0])
    both(gc.edited(box, lambda g, xp: xp.__setitem__((tr, 0), xp[tr, 0] + 10.0)))               # a Translate's offset
    both(gc.edited(box, lambda g, xp: xp.__setitem__(ro, (np.sin(0.3), np.cos(0.3), xp[ro, 2]))))  # a RotateY's sin and cos
    both(gc.edited(box, lambda g, xp: g.__setitem__((0, 4), g[0, 4] - 5.0)))                    # a rectangle's plane
    tri = fl.flatten(SCENES["triangles"]())
    t = int(np.flatnonzero(gc.kinds(tri) == fl.PRIM_TRIANGLE)[0])
    both(tri)
    both(gc.edited(tri, lambda g, xp: g.__setitem__((t, 1), g[t, 1] + 0.1)))                    # a vertex
    fog = fl.flatten(SCENES["cornell-fog"]())
    b = int(np.flatnonzero((np.asarray(fog.prim_kind) & fl.PRIM_BOUNDARY) != 0)[0])
    both(fog)
    both(gc.edited(fog, lambda g, xp: g.__setitem__((b, 0), g[b, 0] + 1.0)))                    # a boundary primitive


def test_the_hook_applies_creation_checks():
    fog = fl.flatten(SCENES["cornell-fog"]())
    medium = int(np.flatnonzero(gc.kinds(fog) == fl.PRIM_MEDIUM)[0])
    for change in (lambda g, xp: g.__setitem__((medium, 0), np.nan), lambda g, xp: g.__setitem__((medium, 2), 1000.0)):
        f = gc.edited(fog, change)
        assert gc.pack_geometry_hash(f, 0)[0] == gc.pack_geometry_hash(f, 1)[0] == RTMI_E_ARG
        assert "medium" in _ffi.lib().rtmi_last_error().decode()


# ---- the refit ----------------------------------------------------------------------------------------------------------------------------------
def test_refit_half_rounding_is_the_builders():
    L = _ffi.lib()
    rng = np.random.default_rng(5)
    vals = np.concatenate([rng.standard_normal(2000) * 10.0 ** rng.integers(-12, 6, 2000), [0.0, -0.0, 65504.0, 65505.0, -65520.0, 1e30, -1e30, np.inf, -np.inf,
                           2.0 ** -14, 2.0 ** -24, 2.0 ** -25, 2.0 ** -24 * 1.5, 2.0 ** -14 - 2.0 ** -26, 1e-40, -1e-44, 6.1e-5, 1023.9 * 2.0 ** -24]])
    for v in vals.astype(np.float32):
        for up in (0, 1):
            assert L.rtmi_test_refit_half(float(v), up) == L.rtmi_test_half_outward(float(v), up), (float(v), up)


def _cornell_edit(flat):
    """a block's Translate offset and RotateY angle, a wall moved, within the box"""
    tr = int(np.flatnonzero(flat.xform_kind == fl.XFORM_TRANSLATE)[0])
    ro = int(np.flatnonzero(flat.xform_kind == fl.XFORM_ROTATE_Y)[-1])

    def change(g, xp):
        xp[tr, 0] += 7.0
        xp[tr, 2] -= 11.0
        a = np.arctan2(xp[ro, 0], xp[ro, 1]) + 0.1
        xp[ro, 0], xp[ro, 1] = np.sin(a), np.cos(a)
        lamp = int(np.flatnonzero(gc.kinds(flat) == fl.PRIM_RECT_XZ)[0])
        g[lamp, 0] += 3.0
        g[lamp, 2] += 3.0
    return gc.edited(flat, change)


def _chain_edit(flat):
    """every sphere of the chain a tenth smaller and a thousandth nearer the origin"""
    which = np.flatnonzero(np.abs(flat.prim_geom[:, 3]) < 1.0)

    def change(g, xp):
        g[which, 0:3] *= 0.999
        g[which, 3] *= 0.9
    return gc.edited(flat, change)


def _lone():
    H, S, T, _ = ts._mods()
    mats, light = ts._materials()
    return fl.flatten(ts.scene([ts._dome(light), H.sphere(center=np.array([1.5, 0.0, 0.0]), radius=0.5, material=mats[0])]))


REFIT_SCENES = {
    "cover": (gc.cover, lambda f: gc.shrink_and_nudge(f, gc.small_spheres(f)[::3])),
    "cornell": (lambda: fl.flatten(r.scene.make_cornell_box(36, 20)), _cornell_edit),
    "lone": (_lone, lambda f: gc.edited(f, lambda g, xp: g.__setitem__(1, g[1] * 0.75))),
    "chain-depth-29": (lambda: fl.flatten(ts.chain_scene(ts.chain(1000, 0.9, 0.15))), _chain_edit),
}


@pytest.fixture(scope="module")
def refit_scenes():
    return {name: (make(), edit) for name, (make, edit) in REFIT_SCENES.items()}


@pytest.mark.parametrize("node16", [0, 1])
@pytest.mark.parametrize("name", sorted(REFIT_SCENES))
def test_refit_is_the_builders_array_and_numpys(refit_scenes, monkeypatch, name, node16):
    monkeypatch.setenv("RTMI_NODE16", str(node16))
    A, edit = refit_scenes[name]
    B = edit(A)
    built, same, moved = gc.refit([A]), gc.refit([A, A]), gc.refit([A, B])
    assert (built["rc"], same["rc"], moved["rc"]) == (0, 0, 0)
    assert built["node16"] == same["node16"] == moved["node16"] == node16 and built["records"] > 0
    if name == "cover":
        assert built["grid_n"] > 0 and built["tall"] != gc.BVH_EMPTY  # an entry grid was built
    if name == "chain-depth-29":
        assert built["launches"] == 0 and same["launches"] == ts.HOST_TABLE["chain(1000, 0.9, 0.15)"][1]  # one launch per height: the tree is 29 deep
    if name == "lone":
        assert built["records"] == 1
    for out in (same, moved):
        assert (out["rebuilt"], out["rebuilds"], out["displaced"]) == (0, 0, 0), name
        assert out["records"] == built["records"] and out["launches"] >= 1
    # (a) nothing moved: the refit is the build, byte for byte (the builder's rounding commutes with min / max)
    assert np.array_equal(same["nodes"], built["nodes"])
    # (b) something moved: an independent bottom-up recomputation from the leaf boxes
    assert not np.array_equal(moved["nodes"], built["nodes"])
    want, have = gc.numpy_refit(moved["nodes"], node16, moved["leaf_box"])
    assert np.array_equal(want, have)
    assert np.array_equal(*gc.numpy_refit(same["nodes"], node16, same["leaf_box"]))
    # (c) the topology is untouched: child codes, roots, the grid's root codes, the big list
    for out in (same, moved):
        assert np.array_equal(gc.child_codes(out["nodes"], node16), gc.child_codes(built["nodes"], node16))
        assert (out["root"], out["tall"], out["grid_n"], out["big"]) == (built["root"], built["tall"], built["grid_n"], built["big"])
        assert np.array_equal(out["cells"], built["cells"])
    # the leaf boxes: every tree primitive's box holds its sphere, everything else is empty
    if name in ("cover", "chain-depth-29"):
        lb, g = moved["leaf_box"], B.prim_geom
        inside = np.isfinite(lb[:, 0])
        assert inside.sum() == len(lb) - built["n_big"]
        assert np.all(lb[inside, :3] < (g[inside, :3] - np.abs(g[inside, 3:4]))) and np.all(lb[inside, 3:] > (g[inside, :3] + np.abs(g[inside, 3:4])))
        assert np.all(lb[~inside, :3] == np.inf) and np.all(lb[~inside, 3:] == -np.inf)


# ---- the fit and displacement rules ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cover():
    A = gc.cover()
    return A, gc.refit([A], want_nodes=False)


def _verdict(steps):
    out = gc.refit(steps)
    assert out["rc"] == 0, out
    return out


def test_fit_rule_bounds(cover):
    A, built = cover
    g = A.prim_geom
    small = gc.small_spheres(A)
    assert built["big"] == [0, 1]  # the ground and the sky dome, out of the tree
    # the trees' coordinate bound: the tree primitive that reaches farthest may shrink, not grow
    reach = np.abs(g[small, :3]).max(axis=1) + np.abs(g[small, 3])
    far = int(small[np.argmax(reach)])
    assert _verdict([A, gc.edited(A, lambda q, xp: q.__setitem__((far, 3), q[far, 3] * 0.99))])["rebuilt"] == 0
    assert _verdict([A, gc.edited(A, lambda q, xp: q.__setitem__((far, 3), q[far, 3] * 1.5))])["rebuilt"] == 1
    # the scene bound: a big primitive (never a tree item) may grow while it stays inside 1.001 x the built bound
    big = int(np.argmax(np.abs(g[:, 3])))
    assert big in built["big"]
    reach_big = np.abs(g[big, :3]).max() + abs(g[big, 3])
    inside = _verdict([A, gc.edited(A, lambda q, xp: q.__setitem__((big, 3), q[big, 3] + 5e-4 * reach_big))])
    assert (inside["rebuilt"], inside["displaced"], inside["big"]) == (0, 0, built["big"])
    assert _verdict([A, gc.edited(A, lambda q, xp: q.__setitem__((big, 3), q[big, 3] + 2e-3 * reach_big))])["rebuilt"] == 1
    # a primitive that can no longer be bounded
    assert _verdict([A, gc.edited(A, lambda q, xp: q.__setitem__((far, 0), np.inf))])["rebuilt"] == 1


def _carry(A, which, lift=1.0):
    """spheres `which` carried to the far side of the layer (x and z mirrored) and lifted above it"""
    def change(q, xp):
        for i in which:
            q[i, 0], q[i, 2] = -q[i, 0] * 0.5, -q[i, 2] * 0.5
            q[i, 1] += lift
    return gc.edited(A, change)


def test_displacement_and_the_big_list(cover):
    A, built = cover
    small = gc.small_spheres(A)
    room = 16 - built["n_big"]
    one = _verdict([A, _carry(A, small[:1])])
    assert (one["rebuilt"], one["displaced"], one["big"]) == (0, 1, sorted(built["big"] + [int(small[0])]))
    assert np.all(one["leaf_box"][small[0], :3] == np.inf)  # its leaves are empty boxes in every tree that holds it
    assert np.array_equal(*gc.numpy_refit(one["nodes"], one["node16"], one["leaf_box"]))
    # moved again, even back home: still displaced (once out, out until a rebuild); the big list stays ascending
    back = _verdict([A, _carry(A, small[:1]), A])
    assert (back["rebuilt"], back["displaced"], back["big"]) == (0, 1, one["big"])
    pick = small[::-1][:room]  # (descending on purpose: the list is sorted by index, not by arrival)
    full = _verdict([A, _carry(A, pick)])
    assert (full["rebuilt"], full["displaced"], full["n_big"]) == (0, room, 16) and full["big"] == sorted(full["big"])
    over = _verdict([A, _carry(A, small[::-1][:room + 1])])
    assert (over["rebuilt"], over["displaced"], over["big"]) == (1, 0, built["big"]) or (over["rebuilt"], over["displaced"]) == (1, 0)
    # one at a time: the seventeenth entry rebuilds, and the rebuild forgets every displacement
    steps = [A] + [_carry(A, small[:k]) for k in range(1, room + 2)]
    seq = _verdict(steps)
    assert (seq["rebuilt"], seq["rebuilds"], seq["displaced"]) == (1, 1, 0)


def test_displacement_compares_the_built_range(cover):
    A, built = cover
    small = gc.small_spheres(A)
    i = int(small[np.argmin(np.abs(A.prim_geom[small, 0]) + np.abs(A.prim_geom[small, 2]))])  # in the middle of the layer: far from the trees' bound
    shrunk = gc.edited(A, lambda q, xp: q.__setitem__((i, 3), q[i, 3] * 0.25))
    home = _verdict([A, shrunk, A])  # shrink, then grow back: the box it was built with
    assert (home["rebuilt"], home["displaced"]) == (0, 0)
    assert np.array_equal(home["nodes"], gc.refit([A])["nodes"])
    grown = gc.edited(A, lambda q, xp: q.__setitem__((i, 3), 3.0))  # across several cells and out of the layer
    assert _verdict([A, shrunk, grown])["displaced"] == 1
    # within the layer's height but into cells it was not registered in: a slide of two cell widths along x
    slid = gc.edited(A, lambda q, xp: q.__setitem__((i, 0), q[i, 0] + (2.5 if q[i, 0] < 0 else -2.5)))
    assert _verdict([A, slid])["displaced"] == 1
    # a tall primitive (one of the three unit spheres) leaves the tall primitives' box upwards
    tall = int(np.flatnonzero(np.abs(A.prim_geom[:, 3]) == 1.0)[0])
    assert _verdict([A, gc.edited(A, lambda q, xp: q.__setitem__((tall, 3), 0.9))])["displaced"] == 0
    assert _verdict([A, gc.edited(A, lambda q, xp: q.__setitem__((tall, 1), q[tall, 1] + 0.5))])["displaced"] == 1


def test_scenes_without_a_grid_never_displace():
    A = fl.flatten(r.scene.make_random_scene(36, 20, 3, False))
    built = gc.refit([A])
    assert built["grid_n"] == 0
    small = gc.small_spheres(A)
    i, j = int(small[0]), int(small[-1])

    def swap(q, xp):
        q[[i, j], 0:3] = q[[j, i], 0:3]
    out = _verdict([A, gc.edited(A, swap)])
    assert (out["rebuilt"], out["displaced"], out["big"]) == (0, 0, built["big"])
    assert np.array_equal(*gc.numpy_refit(out["nodes"], out["node16"], out["leaf_box"]))


def test_experiment_knobs_and_media_rows_rebuild(monkeypatch):
    H, S, T, _ = ts._mods()
    mats, light = ts._materials()
    items = [ts._dome(light)] + [H.translate(item=H.box(p0=(0.0, 0.0, 0.0), p1=(0.5, 0.6, 0.7), material=mats[k % 3]), offset=(1.0 + k, -0.3, 0.2 * k)) for k in range(3)]
    box = fl.flatten(ts.scene(items))
    tr = int(np.flatnonzero(box.xform_kind == fl.XFORM_TRANSLATE)[0])
    B = gc.edited(box, lambda g, xp: xp.__setitem__((tr, 1), xp[tr, 1] + 0.25))
    assert _verdict([box, B])["rebuilt"] == 0
    monkeypatch.setenv("RTMI_BOX_LEAF", "1")
    assert _verdict([box, B])["rebuilt"] == 1  # one leaf over six faces has no box of its own in leaf_box
    monkeypatch.delenv("RTMI_BOX_LEAF")
    fog = fl.flatten(r.scene.make_cornell_box(36, 20, classic=False))
    medium = int(np.flatnonzero(gc.kinds(fog) == fl.PRIM_MEDIUM)[0])
    wall = int(np.flatnonzero(gc.kinds(fog) == fl.PRIM_RECT_XZ)[0])
    moved = gc.edited(fog, lambda g, xp: g.__setitem__((wall, 0), g[wall, 0] + 3.0))
    assert _verdict([fog, moved])["rebuilt"] == 0
    assert _verdict([fog, gc.edited(fog, lambda g, xp: g.__setitem__((medium, 0), g[medium, 0] * 2.0))])["rebuilt"] == 1  # a medium's density is structure
    # media neighbourhood trees: a small ball of fog among a row of spheres
    ball = H.constant_medium(boundary=H.sphere(center=np.array([2.0, 0.0, 0.0]), radius=0.45, material=mats[0]), density=0.5, albedo=T.constant(color=np.ones(3)))
    row = [H.sphere(center=np.array([1.0 + k, 0.0, 0.0]), radius=0.2, material=mats[k % 3]) for k in range(8)]
    haze = fl.flatten(ts.scene([ts._dome(light)] + row + [ball]))
    last = int(gc.small_spheres(haze)[7])
    moved = gc.edited(haze, lambda g, xp: g.__setitem__((last, 1), g[last, 1] + 0.125))
    plain = gc.refit([haze])
    assert _verdict([haze, moved])["rebuilt"] == 0
    monkeypatch.setenv("RTMI_MLOC", "1")
    assert gc.refit([haze])["records"] > plain["records"]  # the build made a neighbourhood tree for the ball
    assert _verdict([haze, moved])["rebuilt"] == 1
