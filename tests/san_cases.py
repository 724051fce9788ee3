"""Cases for the sanitized builds of the library's host half (tests/test_host_sanitizers.py, tests/host_san/driver.cpp).  Not a test module.

A CALL names one host-only hook of include/rtmi.h, a label and the hook's arguments as numpy arrays (an int: a scalar; None: the pointer is NULL).
`write_cases` puts a list of calls into the case file the stand-alone driver reads; `expected_line` makes the same call on the ordinary librtmi.so,
through ctypes, and formats what it returned exactly as the driver does -- the sanitized build must print the same line.  Every output buffer is
filled with PATTERN bytes first and reported whole, so a failing call shows that it wrote nothing.

The inputs are the ones the host tests already build (tree_scenes, geometry_cases, direct_cases, the scenes and tables of test_materials_host,
test_geometry_host, test_stage_host), marshalled by core.scene_arrays.  Nothing here loads a library: the caller passes it in."""
import copy
import ctypes as C
import struct

import numpy as np

import raytrace_clj_amd as r
from raytrace_clj_amd import core
from raytrace_clj_amd import flatten as fl
import direct_cases as dcs
import geometry_cases as gc
import tree_scenes as ts

PATTERN = 0xA5
DIRECT_MAX_LIGHTS = 32
_TYPES = {np.dtype(np.uint8): 0, np.dtype(np.int32): 1, np.dtype(np.int64): 2, np.dtype(np.uint64): 3, np.dtype(np.float64): 4}


class Call:
    def __init__(self, kind, label, fails=False, **args):
        assert " " not in kind and " " not in label and "\n" not in label  # (the driver's lines are split at spaces)
        # fails: the return code the hook must refuse this input with (True: any code but 0; False: the input is sound)
        self.kind, self.label, self.fails = kind, label, fails
        self.args = {k: v for k, v in args.items() if v is not None}

    def arr(self, name):
        v = self.args.get(name)
        return None if v is None else np.ascontiguousarray(v)

    def num(self, name, otherwise=0):
        return int(self.args.get(name, otherwise))


def write_cases(path, calls):
    def record(f, name, a):
        a = np.ascontiguousarray(a)
        f.write(struct.pack("<I", len(name)) + name.encode() + struct.pack("<IQ", _TYPES[a.dtype], a.size) + a.tobytes())

    with open(path, "wb") as f:
        for c in calls:
            record(f, "call", np.frombuffer(("%s %s" % (c.kind, c.label)).encode(), np.uint8))
            for name, v in c.args.items():
                record(f, name, np.array([v], np.int64) if isinstance(v, (int, np.integer)) else v)


# ---- the driver's formats ---------------------------------------------------------------------------------------------------------------------------
def fnv1a(data):
    h = 1469598103934665603
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def _num(key, v):
    return " %s=%d" % (key, int(v))


def _hex(key, v):
    return " %s=%016x" % (key, int(v))


def _list(key, a, as_hex=False):
    if a is None:
        return " %s=null" % key
    return " %s=[%s]" % (key, ",".join(("%x" if as_hex else "%d") % int(v) for v in a))


def _hash(key, a):
    return " %s=null" % key if a is None else _hex(key, fnv1a(a.tobytes()))


def _out(count, dtype):
    """count elements of the pattern (0 or less: no buffer, a NULL pointer)"""
    if count <= 0:
        return None
    a = np.empty(int(count), dtype)
    a.view(np.uint8)[:] = PATTERN
    return a


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def expected_line(L, c):
    """the line the driver prints for call c, computed with library L (the ordinary librtmi.so, bound by _ffi.lib()); a refused call's text comes last"""
    err = []
    return _expected_fields(L, c, err) + "".join(err)


def _expected_fields(L, c, err):
    keep = {name: c.arr(name) for name in c.args if not isinstance(c.args[name], (int, np.integer))}  # (contiguous copies: alive during the call)
    p = lambda name: _p(keep.get(name))  # noqa: E731
    s = "%s %s" % (c.label, c.kind)

    def rc(code):
        if code != 0:
            err.append(" err=" + L.rtmi_last_error().decode())
        return _num("rc", code)

    k = c.kind
    if k == "build_tree":
        h, info, ms = _out(1, np.uint64), _out(4, np.int32), _out(1, np.float64)
        code = L.rtmi_test_build_tree(c.num("n"), p("geom"), p("cam"), c.num("threads"), None if c.num("no_hash") else _p(h), _p(info), _p(ms))
        return s + rc(code) + _hex("hash", h[0]) + _list("info", info)
    if k == "pack_materials":
        h, facts = _out(1, np.uint64), _out(3, np.int32)
        args = tuple(_p(keep.get(n)) if isinstance(n, str) else n for n in _scene_names(c))
        code = L.rtmi_test_pack_materials(*args, c.num("through_creation"), _p(h), _p(facts))
        return s + rc(code) + _hex("hash", h[0]) + _list("facts", facts)
    if k == "pack_geometry":
        h = _out(1, np.uint64)
        args = tuple(_p(keep.get(n)) if isinstance(n, str) else n for n in _scene_names(c))
        code = L.rtmi_test_pack_geometry(*args, c.num("through_creation"), _p(h))
        return s + rc(code) + _hex("hash", h[0])
    if k == "refit":
        cap, cells_cap, leaf_floats = c.num("capacity", -1), c.num("cells_capacity", -1), c.num("leaf_floats")
        nodes, cells, leaf, big = _out(cap, np.uint8), _out(cells_cap, np.int32), _out(leaf_floats, np.float32), _out(16 if c.num("want_big") else 0, np.int32)
        nbytes, info = _out(1, np.int64), _out(10, np.int32)
        code = L.rtmi_test_refit(c.num("n_prims"), p("prim_kind"), p("prim_flip"), p("prim_xform"), c.num("n_xforms"), p("xform_kind"), c.num("cam_kind"), p("cam"),
                                 c.num("n_steps"), p("geoms"), p("xforms"), _p(nodes), max(cap, 0), _p(nbytes), _p(info), _p(big), _p(cells), max(cells_cap, 0), _p(leaf))
        return s + rc(code) + _num("bytes", nbytes[0]) + _list("info", info) + _list("big", big) + _hash("nodes", nodes) + _hash("cells", cells) + _hash("leaf_box", leaf)
    if k == "scene_lights":
        cap = c.num("capacity")
        prims, count = _out(c.num("alloc", cap), np.int32), _out(1, np.int32)
        code = L.rtmi_test_scene_lights(c.num("n_prims"), p("prim_kind"), p("prim_geom"), p("prim_mat"), c.num("n_mats"), p("mat_kind"), p("mat_tex"), c.num("n_tex"),
                                        p("tex_kind"), p("prim_xform"), cap, _p(prims), None if c.num("no_count") else _p(count))
        return s + rc(code) + _num("count", count[0]) + _list("prims", prims)
    if k == "stage_layout":
        n_alloc = len(keep["elem_bytes"]) if "elem_bytes" in keep else 0
        off, total = _out(n_alloc, np.uint64), _out(1, np.uint64)
        code = L.rtmi_test_stage_layout(c.num("n"), p("elem_bytes"), p("counts"), p("present"), _p(off), _p(total))
        return s + rc(code) + _hex("total", total[0]) + _list("offsets", off, True)
    if k == "halves":
        out = []
        for x in keep["x"]:
            out += [L.rtmi_test_half_outward(float(x), 0), L.rtmi_test_half_outward(float(x), 1), L.rtmi_test_refit_half(float(x), 0), L.rtmi_test_refit_half(float(x), 1)]
        return s + _list("half", out)
    if k == "camera_fixed":
        return s + _num("flags", L.rtmi_test_camera_fixed(c.num("cam_kind"), p("cam")))
    if k == "sample_keys":
        return s + _list("keys", [L.rtmi_sample_key(int(a), int(b), int(d)) for a, b, d in zip(keep["seed"], keep["pixel"], keep["sample"])], True)
    if k == "version":
        return s + _num("version", L.rtmi_version())
    raise ValueError(k)


def _scene_names(c):
    """creation's nineteen arguments: a string names an array of the call, an int is the count itself"""
    return (c.num("n_prims"), "prim_kind", "prim_geom", "prim_mat", c.num("n_mats"), "mat_kind", "mat_tex", "mat_param", c.num("n_tex"), "tex_kind", "tex_param",
            "tex_child", c.num("cam_kind"), "cam", "prim_flip", "prim_xform", c.num("n_xforms"), "xform_kind", "xform_param")


def line_fields(line):
    """a driver line -> (label, kind, {key: value} of its output fields, the error text or None)"""
    head, _, text = line.partition(" err=")
    words = head.split(" ")
    return words[0], words[1], dict(w.split("=", 1) for w in words[2:]), (text if " err=" in line else None)


def buffer_bytes(c):
    """the sizes in bytes of the whole buffers a refit call's line reports by hash"""
    return {"nodes": c.num("capacity", -1), "cells": 4 * c.num("cells_capacity", -1), "leaf_box": 4 * c.num("leaf_floats")}


def wrote_nothing(line, c):
    """every output the line of call c reports still holds the pattern: scalars and lists element by element, the refit's whole buffers by the FNV-1a
    of the pattern at the buffer's size"""
    fields = line_fields(line)[2]
    i32 = int.from_bytes(bytes([PATTERN] * 4), "little", signed=True)
    i64, u64 = int.from_bytes(bytes([PATTERN] * 8), "little", signed=True), "%016x" % int.from_bytes(bytes([PATTERN] * 8), "little")
    outputs = 0
    for key, v in fields.items():
        if key == "rc" or v == "null":
            continue
        outputs += 1
        if key in ("hash", "total"):
            ok = v == u64
        elif key in ("nodes", "cells", "leaf_box"):
            ok = v == "%016x" % fnv1a(bytes([PATTERN]) * buffer_bytes(c)[key])
        elif key == "offsets":
            ok = all(x == u64 for x in v.strip("[]").split(",") if x)
        elif key == "bytes":
            ok = int(v) == i64
        else:
            ok = all(int(x) == i32 for x in v.strip("[]").split(",") if x)
        if not ok:
            return False
    return outputs > 0


# ---- marshalling ------------------------------------------------------------------------------------------------------------------------------------
def scene_call(kind, label, flat, through_creation, fails=False, drop=(), **over):
    """rtmi_test_pack_materials / rtmi_test_pack_geometry over a FlatScene (drop: arrays passed as NULL; over: arguments replaced)"""
    a, _ = core.scene_arrays(flat)
    args = dict(a, n_prims=len(a["prim_kind"]), n_mats=len(a["mat_kind"]), n_tex=len(a["tex_kind"]), cam_kind=int(flat.cam_kind), n_xforms=len(a["xform_kind"]),
                through_creation=through_creation)
    for name in drop:
        args[name] = None
    args.update(over)
    return Call(kind, label, fails, **args)


def camera(at=ts.CAMERA_AT):
    cam = np.zeros(24, np.float64)
    cam[:3] = at
    return cam


def tree_call(label, spheres, threads, fails=False, **over):
    spheres = np.ascontiguousarray(spheres, np.float64)
    args = dict(n=len(spheres), geom=spheres.reshape(-1), cam=camera(), threads=threads)
    args.update(over)
    return Call("build_tree", label, fails, **args)


def refit_call(label, steps, sizes=None, outputs="all", short=False, fails=False, **over):
    """rtmi_test_refit over FlatScenes of one structure.  sizes: (node bytes, grid cells, world primitives) of the result, from refit_sizes;
    outputs "all": every optional output at exactly its size, "none": every optional output NULL; short: the node array and the grid's cells get one
    element less than they need (the entry reports the size and must write nothing past the end)."""
    f0 = steps[0]
    a = lambda x, dt: np.ascontiguousarray(x, dt)  # noqa: E731
    n = len(f0.prim_kind)
    xk = a(f0.xform_kind, np.int32)
    args = dict(n_prims=n, prim_kind=a(f0.prim_kind, np.int32), prim_flip=a(f0.prim_flip, np.int32), prim_xform=a(f0.prim_xform, np.int32).reshape(-1),
                n_xforms=len(xk), xform_kind=xk if len(xk) else None, cam_kind=int(f0.cam_kind), cam=a(f0.cam, np.float64), n_steps=len(steps),
                geoms=a(np.stack([np.asarray(f.prim_geom, np.float64).reshape(n, -1) for f in steps]), np.float64).reshape(-1),
                xforms=a(np.stack([np.asarray(f.xform_param, np.float64).reshape(-1, 3) for f in steps]), np.float64).reshape(-1) if len(xk) else None)
    if outputs == "all":
        nbytes, cells, n_world = sizes
        args.update(capacity=nbytes - (1 if short else 0), cells_capacity=cells - (1 if short and cells else 0), leaf_floats=6 * n_world, want_big=1)
    args.update(over)
    return Call("refit", label, fails, **args)


def refit_sizes(steps):
    """(node bytes, grid cells, world primitives) of the state after the last step, by a sizing call of the ordinary library"""
    out = gc.refit(steps, want_nodes=True)
    assert out["rc"] == 0, out
    return len(out["nodes"]), len(out["cells"]), len(out["leaf_box"])


def lights_call(label, f, capacity, fails=False, **over):
    i32 = lambda x: np.ascontiguousarray(x, np.int32)  # noqa: E731
    kind = i32(f.prim_kind)
    chains = getattr(f, "prim_xform", None)
    args = dict(n_prims=len(kind), prim_kind=kind, prim_geom=np.ascontiguousarray(f.prim_geom, np.float64).reshape(-1), prim_mat=i32(f.prim_mat),
                n_mats=len(f.mat_kind), mat_kind=i32(f.mat_kind), mat_tex=i32(f.mat_tex), n_tex=len(f.tex_kind), tex_kind=i32(f.tex_kind),
                prim_xform=i32(chains).reshape(-1) if chains is not None and len(chains) == len(kind) else None, capacity=capacity)
    args.update(over)
    return Call("scene_lights", label, fails, **args)


def layout_call(label, planes, fails=False, **over):
    elem, count, present = (np.array([q[k] for q in planes], dt) for k, dt in ((0, np.uint64), (1, np.uint64), (2, np.int32)))
    args = dict(n=len(planes), elem_bytes=elem, counts=count, present=present)
    args.update(over)
    return Call("stage_layout", label, fails, **args)


def edited_tables(flat, change):
    """a copy of `flat` whose material, texture and kind tables `change(copy)` may write"""
    f = copy.copy(flat)
    for name in ("prim_kind", "prim_mat", "prim_xform", "mat_kind", "mat_tex", "mat_param", "tex_kind", "tex_param", "tex_child", "xform_kind"):
        setattr(f, name, np.array(getattr(flat, name), copy=True))
    change(f)
    return f


# ---- a. trees ---------------------------------------------------------------------------------------------------------------------------------------
def tree_cases():
    out = []
    base = ts.sphere_geom(ts.cloud(40, dome=False))
    geoms = [(name, ts.sphere_geom(ts.build(name))) for name in sorted(ts.HOST_TABLE)]
    geoms += [("unboundable[%d]" % k, np.concatenate([base, ts.UNBOUNDABLE[k:k + 1]])) for k in range(len(ts.UNBOUNDABLE))]
    geoms += [("unboundable[all x 3]", np.concatenate([ts.UNBOUNDABLE, base, ts.UNBOUNDABLE, ts.UNBOUNDABLE]))]
    geoms += [("n=%d" % n, base[:n]) for n in (1, 2, 3)]
    geoms += [("scene_sized(20)", ts.scene_sized(20))]
    for name, g in geoms:
        for threads in (1, 0):
            out.append(tree_call("tree/%s/threads=%d" % (name.replace(" ", ""), threads), g, threads))
    return out


# ---- b. geometry packers ------------------------------------------------------------------------------------------------------------------------------
def _scenes():
    from test_materials_host import SCENES
    return {name: fl.flatten(make()) for name, make in sorted(SCENES.items())}


def geometry_cases(scenes=None):
    scenes = scenes or _scenes()
    H, S, T, _ = ts._mods()
    mats, light = ts._materials()
    worlds = dict(scenes)
    worlds["final"] = fl.flatten(r.scene.make_final(36, 20, r.scene.synthetic_earth(32, 16)))
    worlds["mixed(64)"], worlds["mixed(65)"] = fl.flatten(ts.scene(ts.mixed(64))), fl.flatten(ts.scene(ts.mixed(65)))
    worlds["cover-9-moving"] = gc.cover(moving=True)
    worlds["chain_ext"] = fl.flatten(ts.scene(ts.chain_ext(60, 0.9, 0.15)))  # boxes and translate(rotate_y(sphere)) chains among spheres
    # the edits test_geometry_host makes, one of each kind
    cover, box, tri, fog = scenes["cover-moving"], scenes["cornell"], scenes["triangles"], scenes["cornell-fog"]
    moving, static = int(np.flatnonzero(gc.kinds(cover) == fl.PRIM_MOVING)[0]), int(gc.small_spheres(cover)[0])
    tr, ro = int(np.flatnonzero(box.xform_kind == fl.XFORM_TRANSLATE)[0]), int(np.flatnonzero(box.xform_kind == fl.XFORM_ROTATE_Y)[0])
    t = int(np.flatnonzero(gc.kinds(tri) == fl.PRIM_TRIANGLE)[0])
    b = int(np.flatnonzero((np.asarray(fog.prim_kind) & fl.PRIM_BOUNDARY) != 0)[0])
    worlds["cover-moving/centre"] = gc.edited(cover, lambda g, xp: g.__setitem__((static, 0), g[static, 0] + 0.25))
    worlds["cornell/plane"] = gc.edited(box, lambda g, xp: g.__setitem__((0, 4), g[0, 4] - 5.0))
    worlds["cover-moving/radius"] = gc.edited(cover, lambda g, xp: g.__setitem__((static, 3), g[static, 3] * 0.5))
    worlds["cover-moving/center1"] = gc.edited(cover, lambda g, xp: g.__setitem__((moving, 5), g[moving, 5] + 0.125))
    worlds["cornell/translate"] = gc.edited(box, lambda g, xp: xp.__setitem__((tr, 0), xp[tr, 0] + 10.0))
    worlds["cornell/rotate"] = gc.edited(box, lambda g, xp: xp.__setitem__(ro, (np.sin(0.3), np.cos(0.3), xp[ro, 2])))
    worlds["triangles/vertex"] = gc.edited(tri, lambda g, xp: g.__setitem__((t, 1), g[t, 1] + 0.1))
    worlds["cornell-fog/boundary"] = gc.edited(fog, lambda g, xp: g.__setitem__((b, 0), g[b, 0] + 1.0))
    # geometry that cannot be bounded goes through the packers too: creation accepts it
    worlds["cover/non-finite"] = gc.edited(scenes["cover"], lambda g, xp: (g.__setitem__((2, 0), np.inf), g.__setitem__((3, 3), np.nan)))
    return [scene_call("pack_geometry", "geometry/%s/creation=%d" % (name, way), f, way) for name, f in worlds.items() for way in (0, 1)]


def size_sweep_cases():
    """both packers at every primitive count around the record arrays' padding (the FP32 cull records travel in fours, the small-world scan ends at 64,
    a tree over one or two primitives is its own case): mixed-kind worlds of 1 .. 18, 31 .. 34 and 62 .. 67 primitives, sphere clouds of 1 .. 9 and 15 .. 17,
    with and without moving spheres"""
    H = ts._mods()[0]
    out = []
    for n in list(range(1, 19)) + [31, 32, 33, 34] + list(range(62, 68)):
        f = fl.flatten(ts.scene(ts.mixed(n)))
        out += [scene_call(kind, "sizes/mixed(%d)/%s" % (n, kind), f, 1) for kind in ("pack_geometry", "pack_materials")]
    mats, light = ts._materials()
    for n in list(range(1, 10)) + [15, 16, 17]:
        items = ts.cloud(n, dome=False)
        moving = [H.moving_sphere(center0=it.center, t0=0.0, center1=it.center + (0.0, 0.25, 0.0), t1=1.0, radius=it.radius, material=it.material) if k % 2 else it
                  for k, it in enumerate(items)]
        for name, world in (("cloud", items), ("moving-cloud", moving)):
            f = fl.flatten(ts.scene(world, lens=True))
            out += [scene_call("pack_geometry", "sizes/%s(%d)/creation=%d" % (name, n, way), f, way) for way in (0, 1)]
    return out


# ---- c. material packers ------------------------------------------------------------------------------------------------------------------------------
def nested_textures(depth):
    """one sphere whose texture is a chain of `depth` wrappers (checker, flip u, flip v in turn, children BEFORE and AFTER their parents) over a gradient"""
    f = edited_tables(fl.flatten(r.scene.make_two_spheres(36, 20)), lambda f: None)
    n = depth + 2
    order = list(range(n))
    order[1:-1] = order[1:-1][::2] + order[1:-1][1::2][::-1]  # the chain's links are scattered over the table
    kind, param, child = np.zeros(n, np.int32), np.zeros((n, fl.TEX_STRIDE)), np.full((n, 2), -1, np.int32)
    for link in range(depth):
        t, below = order[link], order[link + 1]
        kind[t] = (fl.TEX_CHECKER, fl.TEX_FLIP_U, fl.TEX_FLIP_V)[link % 3]
        param[t, 0] = 2.0 + link
        child[t] = (below, order[-1]) if kind[t] == fl.TEX_CHECKER else (below, -1)
    kind[order[depth]], param[order[depth]] = fl.TEX_UVGRADIENT, np.arange(12) / 12.0
    kind[order[-1]], param[order[-1], :3] = fl.TEX_CONSTANT, (0.5, 0.25, 0.125)
    f.tex_kind, f.tex_param, f.tex_child = kind, param, child
    f.mat_tex = np.full(len(f.mat_kind), order[0], np.int32)
    return f


def material_cases(scenes=None):
    scenes = scenes or _scenes()
    out = []
    for name, f in scenes.items():
        out += [scene_call("pack_materials", "materials/%s/creation=%d" % (name, way), f, way) for way in (0, 1)]
        out.append(scene_call("pack_materials", "materials/%s/edit-without-geometry" % name, f, 0,
                              drop=("prim_geom", "cam", "prim_flip", "prim_xform", "xform_kind", "xform_param"), cam_kind=0, n_xforms=0))
    for depth in (1, 2, 7, 64):
        out += [scene_call("pack_materials", "materials/nested(%d)/creation=%d" % (depth, way), nested_textures(depth), way) for way in (0, 1)]
    # two checkers that are each other's children: the tables' checks admit it (a child must only differ from its parent), the packer's fixed point ends
    loop = nested_textures(2)
    loop.tex_kind[:2], loop.tex_child[0], loop.tex_child[1] = fl.TEX_CHECKER, (1, 1), (0, 0)
    loop.mat_tex[:] = 0
    out += [scene_call("pack_materials", "materials/checker-loop/creation=%d" % way, loop, way) for way in (0, 1)]
    # no primitives: an edit needs no prim_kind and no prim_mat then
    two = scenes["two-spheres"]
    out.append(scene_call("pack_materials", "materials/no-primitives/edit", two, 0, n_prims=0, drop=("prim_kind", "prim_mat", "prim_geom")))
    out.append(scene_call("pack_materials", "materials/no-tables/edit", two, 0, n_prims=0, n_mats=0, n_tex=0,
                          drop=("prim_kind", "prim_mat", "prim_geom", "mat_kind", "mat_tex", "mat_param", "tex_kind", "tex_param", "tex_child")))
    return out


# ---- d. refit -----------------------------------------------------------------------------------------------------------------------------------------
def refit_sequences():
    """name -> the FlatScenes of one rtmi_test_refit call: the sequences of test_geometry_host"""
    import test_geometry_host as tgh
    seqs = {}
    for name, (make, edit) in sorted(tgh.REFIT_SCENES.items()):
        A = make()
        seqs[name + "/built"], seqs[name + "/same"], seqs[name + "/moved"] = [A], [A, A], [A, edit(A)]
    A = gc.cover()
    small = gc.small_spheres(A)
    built = gc.refit([A], want_nodes=False)
    room = 16 - built["n_big"]
    seqs["cover/displaced-one"] = [A, tgh._carry(A, small[:1])]
    seqs["cover/displaced-and-back"] = [A, tgh._carry(A, small[:1]), A]
    seqs["cover/big-list-full"] = [A, tgh._carry(A, small[::-1][:room])]
    seqs["cover/big-list-over-rebuilds"] = [A, tgh._carry(A, small[::-1][:room + 1])]
    seqs["cover/one-at-a-time"] = [A] + [tgh._carry(A, small[:k]) for k in range(1, room + 2)]
    far = int(small[np.argmax(np.abs(A.prim_geom[small, :3]).max(axis=1) + np.abs(A.prim_geom[small, 3]))])
    seqs["cover/does-not-fit-rebuilds"] = [A, gc.edited(A, lambda q, xp: q.__setitem__((far, 3), q[far, 3] * 1.5))]
    seqs["cover/unboundable-rebuilds"] = [A, gc.edited(A, lambda q, xp: q.__setitem__((far, 0), np.inf))]
    fog = fl.flatten(r.scene.make_cornell_box(36, 20, classic=False))  # boundary primitives behind the world: n_world < n_prims
    wall = int(np.flatnonzero(gc.kinds(fog) == fl.PRIM_RECT_XZ)[0])
    seqs["cornell-fog/wall-moved"] = [fog, gc.edited(fog, lambda g, xp: g.__setitem__((wall, 0), g[wall, 0] + 3.0))]
    return seqs


def refit_cases(seqs=None):
    out = []
    for name, steps in (seqs or refit_sequences()).items():
        sizes = refit_sizes(steps)
        out.append(refit_call("refit/%s/all-outputs" % name, steps, sizes))
        out.append(refit_call("refit/%s/no-optional-output" % name, steps, outputs="none"))
        out.append(refit_call("refit/%s/one-short" % name, steps, sizes, short=True))
    return out


# ---- e. lights ----------------------------------------------------------------------------------------------------------------------------------------
def light_cases(count_of):
    """count_of(FlatScene) -> the number of its lights (the ordinary library's answer sizes the capacities)"""
    scenes = {name: dcs.flat(name) for name in dcs.SCENES}
    scenes.update({"not-a-light/" + name: f for name, f in dcs.not_lights().items()})
    # more lights than one call samples: forty lamps
    many = edited_tables(fl.flatten(ts.scene(ts.cloud(40, dome=False))), lambda f: None)
    many.mat_kind = np.full(len(many.mat_kind), fl.MAT_DIFFUSE_LIGHT, np.int32)
    many.mat_tex = np.full(len(many.mat_kind), int(np.flatnonzero(many.tex_kind == fl.TEX_CONSTANT)[0]), np.int32)
    scenes["forty-lamps"] = many
    out = []
    for name, f in scenes.items():
        n = count_of(f)
        for cap in sorted({0, max(n - 1, 0), n, DIRECT_MAX_LIGHTS}):
            out.append(lights_call("lights/%s/capacity=%d" % (name, cap), f, cap))
    return out


# ---- f. layout and scalars ------------------------------------------------------------------------------------------------------------------------------
HALVES = [0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-44, 2.0 ** -24, 2.0 ** -25, 2.0 ** -24 * 1.5, 2.0 ** -14, 2.0 ** -14 - 2.0 ** -26, 6.1e-5, 1023.9 * 2.0 ** -24,
          65504.0, -65504.0, 65505.0, -65520.0, 1e30, -1e30, np.inf, -np.inf, np.nan, 1.0, -1.0, 1.0 / 3.0]
HALVES += [float(np.nextafter(np.float32(v), np.float32(d))) for v in (65504.0, -65504.0, 2.0 ** -14, 2.0 ** -24) for d in (np.inf, -np.inf)]


def cameras():
    """the cameras of test_camera_generation_host's certificates: (label, kind, cam[24])"""
    f = fl.flatten(r.scene.make_random_scene(40, 24, 3, False))
    cam, kind = np.array(f.cam, np.float64), int(f.cam_kind)
    out = [("cover", kind, cam), ("pinhole", fl.CAM_PINHOLE, cam)]
    for label, k, v in [("open-lens", 21, 0.5), ("nan-u", 12, np.nan)] + [("lleft[%d]=%r" % (k - 3, v), k, v) for k in (3, 4, 5) for v in (-0.0, -1e-60, 0.0)] + \
                       [("origin[%d]=%r" % (k, v), k, v) for k in (0, 1, 2) for v in (-0.0, -1e-60, np.inf)]:
        c = cam.copy()
        c[k] = v
        out.append((label, kind, c))
    return out


def scalar_cases():
    from test_stage_host import LAYOUTS
    out = [layout_call("layout/" + name, planes) for name, planes in sorted(LAYOUTS.items())]
    out.append(Call("stage_layout", "layout/n=0", n=0))
    out.append(layout_call("layout/n=0-with-arrays", [(8, 3, 1)], n=0))
    # byte products that wrap 32 bits, and counts and element sizes that do by themselves
    out.append(layout_call("layout/wraps-32-bits", [(8, 1 << 29, 1), (4, 1 << 30, 1), (1, (1 << 32) + 1, 1), (3, 0x55555556, 1), (1 << 32, 1, 0), (16, (1 << 28) + 1, 1)]))
    out.append(Call("halves", "halves", x=np.array(HALVES, np.float64)))
    rng = np.random.default_rng(5)
    out.append(Call("halves", "halves/random", x=(rng.standard_normal(200) * 10.0 ** rng.integers(-12, 6, 200)).astype(np.float32).astype(np.float64)))
    out += [Call("camera_fixed", "camera/" + label, cam_kind=kind, cam=cam) for label, kind, cam in cameras()]
    keys = np.array([[0, 0, 0], [1, 2, 3], [2 ** 64 - 1, 2 ** 64 - 1, 2 ** 64 - 1], [0x5EED, 40 * 24 - 1, 7], [2 ** 63, 2 ** 31, 2 ** 32]], np.uint64)
    out.append(Call("sample_keys", "sample-keys", seed=keys[:, 0].copy(), pixel=keys[:, 1].copy(), sample=keys[:, 2].copy()))
    out.append(Call("version", "version"))
    return out


# ---- g. error paths -------------------------------------------------------------------------------------------------------------------------------------
E_ARG, E_UNSUPPORTED = -1, -3  # RTMI_E_ARG: a bad argument or a malformed scene; RTMI_E_UNSUPPORTED: a record kind the GPU path does not hold (rtmi.h)


def packer_error_cases(name, f, code, creation_only, **how):
    """One bad input through both packers and both ways, with the code rtmi.h gives it.  rtmi_test_pack_geometry applies creation's checks on both ways;
    rtmi_test_pack_materials applies them with through_creation = 1, and with 0 "only prim_kind, prim_mat and the material and texture tables are read":
    what only creation can see (creation_only: geometry, instancing, camera, the primitive kinds' range) packs there, return code 0."""
    out = []
    for way in (0, 1):
        for kind in ("pack_materials", "pack_geometry"):
            passes = creation_only and kind == "pack_materials" and way == 0
            out.append(scene_call(kind, "error/%s/%s/creation=%d" % (kind, name, way), f, way, fails=False if passes else code, **how))
    return out


def error_cases(scenes=None):
    scenes = scenes or _scenes()
    out = []
    base = ts.sphere_geom(ts.cloud(8, dome=False))
    out.append(tree_call("error/tree/n=0", base, 1, E_ARG, n=0))
    out.append(tree_call("error/tree/n<0", base, 1, E_ARG, n=-3))
    out.append(tree_call("error/tree/geom-null", base, 1, E_ARG, geom=None))
    out.append(tree_call("error/tree/cam-null", base, 0, E_ARG, cam=None))
    out.append(tree_call("error/tree/hash-null", base, 0, E_ARG, no_hash=1))
    fog, box = scenes["cornell-fog"], scenes["cornell"]
    medium = int(np.flatnonzero(gc.kinds(fog) == fl.PRIM_MEDIUM)[0])
    chained = int(np.flatnonzero(np.asarray(box.prim_xform)[:, 1] > 0)[0])
    nested = nested_textures(3)
    checker, flip = int(np.flatnonzero(nested.tex_kind == fl.TEX_CHECKER)[0]), int(np.flatnonzero(nested.tex_kind == fl.TEX_FLIP_U)[0])
    image = int(np.flatnonzero(scenes["earth"].tex_kind == fl.TEX_IMAGE)[0])
    broken = {  # name -> (input, code, only creation can see it): what test_materials_host and test_geometry_host assert a code for, and creation's other refusals
        "mat_tex-out-of-range": (edited_tables(fog, lambda f: f.mat_tex.__setitem__(0, len(fog.tex_kind))), E_ARG, False),
        "mat_tex-negative": (edited_tables(fog, lambda f: f.mat_tex.__setitem__(0, -2)), E_ARG, False),
        "medium-not-isotropic": (edited_tables(fog, lambda f: f.mat_kind.__setitem__(int(fog.prim_mat[medium]), fl.MAT_LAMBERTIAN)), E_ARG, False),
        "prim_mat-out-of-range": (edited_tables(fog, lambda f: f.prim_mat.__setitem__(0, len(fog.mat_kind))), E_ARG, False),
        "prim_mat-negative": (edited_tables(fog, lambda f: f.prim_mat.__setitem__(len(fog.prim_mat) - 1, -1)), E_ARG, False),
        "tex_kind-unknown": (edited_tables(fog, lambda f: f.tex_kind.__setitem__(0, 99)), E_UNSUPPORTED, False),
        "mat_kind-unknown": (edited_tables(fog, lambda f: f.mat_kind.__setitem__(0, -1)), E_UNSUPPORTED, False),
        "tex_child-out-of-range": (edited_tables(nested, lambda f: f.tex_child.__setitem__((checker, 0), 1000)), E_ARG, False),
        "tex_child-is-itself": (edited_tables(nested, lambda f: f.tex_child.__setitem__((flip, 0), flip)), E_ARG, False),
        "image-index-invalid": (edited_tables(scenes["earth"], lambda f: f.tex_param.__setitem__((image, 0), -1.0)), E_ARG, False),
        "prim_kind-unknown": (edited_tables(fog, lambda f: f.prim_kind.__setitem__(0, 9)), E_UNSUPPORTED, True),
        "xform_kind-unknown": (edited_tables(box, lambda f: f.xform_kind.__setitem__(0, 7)), E_UNSUPPORTED, True),
        "prim_xform-out-of-range": (edited_tables(box, lambda f: f.prim_xform.__setitem__((chained, 0), len(box.xform_kind))), E_ARG, True),
        "prim_xform-negative": (edited_tables(box, lambda f: f.prim_xform.__setitem__((chained, 1), -1)), E_ARG, True),
        "medium-density-nan": (gc.edited(fog, lambda g, xp: g.__setitem__((medium, 0), np.nan)), E_ARG, True),
        "medium-range-invalid": (gc.edited(fog, lambda g, xp: g.__setitem__((medium, 2), 1000.0)), E_ARG, True),
        "world-after-boundary": (edited_tables(fog, lambda f: f.prim_kind.__setitem__(0, int(f.prim_kind[0]) | fl.PRIM_BOUNDARY)), E_ARG, True),
    }
    for name, (f, code, creation_only) in broken.items():
        out += packer_error_cases(name, f, code, creation_only)
    two = scenes["two-spheres"]
    for hole in ("prim_kind", "prim_geom", "prim_mat", "mat_kind", "mat_tex", "mat_param", "tex_kind", "tex_param", "tex_child", "cam"):
        out += packer_error_cases(hole + "-null", two, E_ARG, hole in ("prim_geom", "cam"), drop=(hole,))
    for count in ("n_prims", "n_mats", "n_tex", "n_xforms"):
        out += packer_error_cases(count + "-negative", two, E_ARG, count == "n_xforms", **{count: -1})
    out.append(scene_call("pack_geometry", "error/pack_geometry/xforms-null", box, 1, E_ARG, drop=("xform_param",)))
    out.append(scene_call("pack_materials", "error/pack_materials/camera-kind", two, 1, E_UNSUPPORTED, cam_kind=5))
    lamp = dcs.flat("example-light")
    out.append(lights_call("error/lights/capacity<0", lamp, -1, E_ARG))
    out.append(lights_call("error/lights/out-null", lamp, 4, E_ARG, alloc=0))
    out.append(lights_call("error/lights/count-null", lamp, 4, E_ARG, no_count=1))
    out.append(lights_call("error/lights/arrays-null", lamp, 4, E_ARG, prim_kind=None, prim_geom=None, prim_mat=None))
    out.append(lights_call("error/lights/n_mats<0", lamp, 4, E_ARG, n_mats=-1))
    out.append(Call("stage_layout", "error/layout/n=1-null", E_ARG, n=1))
    out.append(Call("stage_layout", "error/layout/n<0", E_ARG, n=-1))
    A = scenes["cover"]
    sizes = refit_sizes([A])
    out.append(refit_call("error/refit/n_prims=0", [A], sizes, fails=E_ARG, n_prims=0))
    out.append(refit_call("error/refit/n_steps=0", [A], sizes, fails=E_ARG, n_steps=0))
    out.append(refit_call("error/refit/geoms-null", [A], sizes, fails=E_ARG, geoms=None))
    out.append(refit_call("error/refit/cam-null", [A], sizes, fails=E_ARG, cam=None))
    out.append(refit_call("error/refit/xforms-null", [box], refit_sizes([box]), fails=E_ARG, xforms=None))
    out.append(refit_call("error/refit/step-1-refused", [fog, broken["medium-density-nan"][0]], refit_sizes([fog]), fails=E_ARG))
    out.append(refit_call("error/refit/step-0-refused", [broken["medium-range-invalid"][0]], refit_sizes([fog]), fails=E_ARG))
    return out


# ---- h. concurrency -------------------------------------------------------------------------------------------------------------------------------------
def concurrent_cases(scenes=None):
    """two files of four calls each: thread t of the driver runs call t, three rounds, all behind one barrier"""
    scenes = scenes or _scenes()
    small, large = ts.sphere_geom(ts.layer(256)), ts.sphere_geom(ts.layer(20000))
    A = gc.cover()
    steps = [A, gc.shrink_and_nudge(A, gc.small_spheres(A)[::3])]
    trees = [tree_call("together/tree/layer(256)/threads=0", small, 0), tree_call("together/tree/layer(20000)/threads=0", large, 0),
             tree_call("together/tree/layer(20000)/threads=1", large, 1), tree_call("together/tree/layer(256)/threads=0/again", small, 0)]
    mixed = [scene_call("pack_geometry", "together/geometry/cornell", scenes["cornell"], 1), refit_call("together/refit/cover", steps, refit_sizes(steps)),
             tree_call("together/tree/layer(256)/threads=0", small, 0), tree_call("together/tree/layer(256)/threads=1", small, 1)]
    return {"trees": trees, "mixed": mixed}


# ---- the oracle (oracle/san_main.c) ------------------------------------------------------------------------------------------------------------------
FLT_MAX = 3.4028234663852886e38
ORACLE_NX, ORACLE_NY, ORACLE_NS, ORACLE_SEED, N_PROBES = 24, 16, 3, 0x5EED0002, 256


def oracle_scene_args(fs):
    """a FlatScene (with its nested world, Perlin tables and images where it has them) as the arrays of the oracle's scene struct, as oracle.py marshals it"""
    i32, f64 = (lambda a: np.ascontiguousarray(a, np.int32).reshape(-1)), (lambda a: np.ascontiguousarray(a, np.float64).reshape(-1))  # noqa: E731
    args = dict(n_prims=len(i32(fs.prim_kind)), prim_kind=i32(fs.prim_kind), prim_geom=f64(fs.prim_geom), prim_mat=i32(fs.prim_mat), n_mats=len(i32(fs.mat_kind)),
                mat_kind=i32(fs.mat_kind), mat_tex=i32(fs.mat_tex), mat_param=f64(fs.mat_param), n_tex=len(i32(fs.tex_kind)), tex_kind=i32(fs.tex_kind),
                tex_param=f64(fs.tex_param), tex_child=i32(fs.tex_child), cam_kind=int(fs.cam_kind), cam=f64(fs.cam))
    tree = getattr(fs, "tree", None)
    if tree is not None:
        args.update(n_nodes=len(i32(tree["kind"])), root=int(tree["root"]), node_kind=i32(tree["kind"]), node_a=i32(tree["a"]), node_d=f64(tree["d"]),
                    node_prim=i32(tree["prim"]), node_children=i32(tree["children"]))
    if getattr(fs, "perlin_vectors", None) is not None:
        args.update(perlin_vec=f64(fs.perlin_vectors), perlin_perm=i32(fs.perlin_perm))
    images = getattr(fs, "images", None) or []
    if images:
        imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
        sizes = [im.size for im in imgs]
        args.update(n_images=len(imgs), image_wh=i32([[im.shape[1], im.shape[0]] for im in imgs]),
                    image_off=np.ascontiguousarray(np.concatenate([[0], np.cumsum(sizes)[:-1]]), np.int64),
                    image_rgb=np.ascontiguousarray(np.concatenate([im.reshape(-1) for im in imgs]), np.uint8))
    return args


class OracleCall(Call):
    def __init__(self, kind, label, fs, **args):
        Call.__init__(self, kind, label, False, **dict(oracle_scene_args(fs), **args))
        self.fs = fs


def oracle_cases(oracle):
    """the entry points oracle.py calls: whole frames of the three golden scenes on 1 and 16 threads, and 256 probes of every kind on those scenes, on
    worlds with Perlin textures, an image and media, and on the worlds and inputs of test_oracle_kat's K2, K4, K8, K11, K12, K13 and K15 (the
    other K tests call entry points oracle.py's scene calls do not go through).  `oracle` (the ordinary library,
    through oracle.py) makes the camera rays the hit, path and scatter probes start from."""
    from oracle.tree import flatten_with_tree
    import test_oracle_kat as kat
    H, S, T = r.hitable, r.shader, r.texture
    golden = {"two_spheres": fl.flatten(r.scene.make_two_spheres(ORACLE_NX, ORACLE_NY)), "cover_n3": fl.flatten(r.scene.make_random_scene(ORACLE_NX, ORACLE_NY, 3, False)),
              "cornell": flatten_with_tree(r.scene.make_cornell_box(ORACLE_NX, ORACLE_NY))}
    out = [OracleCall("render", "oracle/render/%s/threads=%d" % (name, t), fs, nx=ORACLE_NX, ny=ORACLE_NY, ns=ORACLE_NS, depth=50, seed=ORACLE_SEED, nthreads=t)
           for name, fs in golden.items() for t in (1, 16)]
    worlds = dict(golden)
    worlds["cover_n3_moving"] = fl.flatten(r.scene.make_random_scene(ORACLE_NX, ORACLE_NY, 3, True))
    worlds["perlin"] = flatten_with_tree(r.scene.make_two_perlin_spheres(ORACLE_NX, ORACLE_NY))
    worlds["earth"] = flatten_with_tree(r.scene.make_textured_sphere(ORACLE_NX, ORACLE_NY, r.scene.synthetic_earth(32, 16)))
    worlds["cornell_fog"] = flatten_with_tree(r.scene.make_cornell_box(ORACLE_NX, ORACLE_NY, classic=False))
    rng = np.random.default_rng(31)
    for name, fs in worlds.items():
        uv, keys = rng.random((N_PROBES, 2)), rng.integers(0, 2 ** 63, N_PROBES, dtype=np.uint64)
        rays = np.ascontiguousarray(oracle.probe_camera(fs, uv, keys)[:, :7])
        hits = oracle.probe_hit(fs, rays, 0.001, FLT_MAX)
        out.append(OracleCall("probe_camera", "oracle/camera/" + name, fs, n=N_PROBES, uv=uv.reshape(-1), keys=keys))
        out.append(OracleCall("probe_hit", "oracle/hit/" + name, fs, n=N_PROBES, rays=rays.reshape(-1), tmin=np.array([0.001]), tmax=np.array([FLT_MAX])))
        out.append(OracleCall("probe_paths", "oracle/paths/" + name, fs, n=N_PROBES, rays=rays.reshape(-1), keys=keys, ctr0=100, depth=50, max_seg=4))
        out.append(OracleCall("probe_paths", "oracle/paths-no-log/" + name, fs, n=N_PROBES, rays=rays.reshape(-1), keys=keys, ctr0=0, depth=5, max_seg=0))
        uvp = np.concatenate([rng.random((N_PROBES, 2)), rng.normal(0, 7, (N_PROBES, 3))], axis=1)
        uvp[:4, :2] = [(0.0, 0.0), (1.0, 1.0), (1.0, 0.0), (0.0, 1.0)]  # the corners: an ImageMap's last column and row
        for t in range(len(fs.tex_kind))[:6]:
            out.append(OracleCall("probe_texture", "oracle/texture/%s/%d" % (name, t), fs, n=N_PROBES, tex=t, uvp=uvp.reshape(-1)))
        rec = np.concatenate([np.where(hits[:, :1] != 0, hits[:, 3:6], 0.0), np.where(hits[:, :1] != 0, hits[:, 6:9], (0.0, 1.0, 0.0)), hits[:, 9:11]], axis=1)
        for m in range(len(fs.mat_kind))[:8]:
            out.append(OracleCall("probe_scatter", "oracle/scatter/%s/%d" % (name, m), fs, n=N_PROBES, mat=m, rays=rays.reshape(-1), hits=rec.reshape(-1), keys=keys))
    if "cover_n3_moving" in worlds:  # the bvh-node descent beside the Hitlist scan (test_bvh_equals_flat_scan)
        fs = worlds["cover_n3_moving"]
        o = np.tile((13.0, 2.0, 3.0), (N_PROBES, 1)) + rng.normal(0, 0.5, (N_PROBES, 3))
        rays = np.concatenate([o, -o + rng.normal(0, 3.0, (N_PROBES, 3)), rng.random((N_PROBES, 1))], axis=1)
        out.append(OracleCall("probe_hit", "oracle/hit-bvh/cover_n3_moving", fs, n=N_PROBES, rays=rays.reshape(-1), tmin=np.array([0.001]), tmax=np.array([FLT_MAX]), bvh_seed=2))
    # the known-answer worlds
    origin = kat.GRIDPOINTS[5]
    lattice = lambda t_in, t_out: np.array([kat.ray7(origin + d, -d, t_in) for d in kat.DIRECTIONS] + [kat.ray7(origin + d, d, t_out) for d in kat.DIRECTIONS] +  # noqa: E731
                                           [kat.ray7(origin + (1, 1, 0), (-1, 0, 0)), kat.ray7(origin, (1, 1, 1))])
    k2 = kat.world_of(H.sphere(center=origin, radius=1.0, material=kat.MATERIAL))
    k4 = kat.world_of(H.moving_sphere(center0=origin, t0=0.1, center1=origin + (10, 20, 30), t1=0.9, radius=1.0, material=kat.MATERIAL))
    for name, w, rays in (("k2", k2, lattice(0.0, 0.1)), ("k4", k4, lattice(0.1, 0.1))):
        out.append(OracleCall("probe_hit", "oracle/kat/" + name, w, n=len(rays), rays=rays.reshape(-1), tmin=np.array([0.0]), tmax=np.array([FLT_MAX])))
    k8 = kat.world_of(H.sphere(center=np.zeros(3), radius=1.0, material=kat.MATERIAL))
    rays = np.array([kat.ray7((0, 0, -5), (0, 0, 1)), kat.ray7((0, 0, 0), (1, 1, 1)), kat.ray7((1, 1, 0), (-1, 0, 0))], np.float64)
    for tmin, tmax in ((0.0, FLT_MAX), (4.0, FLT_MAX), (0.0, 4.0)):
        out.append(OracleCall("probe_hit", "oracle/kat/k8/%g-%g" % (tmin, tmax), k8, n=len(rays), rays=rays.reshape(-1), tmin=np.array([tmin]), tmax=np.array([tmax])))
    # K11 and K12: the sky dome's texture at the uv of five normals, and the centre ray of the camera, on the cover scene n = 11 at aspect 2
    cover11 = fl.flatten(r.scene.make_random_scene(200, 100, 11, False))
    dome = int(np.flatnonzero(cover11.prim_kind == fl.PRIM_UVSPHERE)[0])
    uvp = np.array([list(oracle.sphere_uv(np.array(n, np.float64))) + [0.0, 0.0, 0.0] for n in ((0, 1, 0), (1, 0, 0), (0, -1, 0), (0, 0, 1), (0.6, 0.8, 0))])
    out.append(OracleCall("probe_texture", "oracle/kat/k11", cover11, n=len(uvp), tex=int(cover11.mat_tex[cover11.prim_mat[dome]]), uvp=uvp.reshape(-1)))
    out.append(OracleCall("probe_camera", "oracle/kat/k12", cover11, n=1, uv=np.array([0.5, 0.5]), keys=np.array([12345], np.uint64)))
    metal, mirror = S.metal(albedo=T.constant(color=np.ones(3)), fuzz=10), S.metal(albedo=T.constant(color=np.ones(3)), fuzz=0.0)
    lam, light = S.lambertian(albedo=T.constant(color=np.full(3, 0.5))), S.diffuse_light(tex=T.constant(color=np.ones(3)))
    k13 = {"dome": (kat.world_of(kat._dome()), kat.ray7((1, 2, 3), (0, -1, 0)), 50),
           "depth-0": (kat.world_of(kat._dome(), H.sphere(center=np.array((0.0, 0.0, -5.0)), radius=1.0, material=kat.MATERIAL)), kat.ray7((0, 0, 0), (0, 0, -1)), 0),
           "fuzz-10": (kat.world_of(kat._dome(), H.sphere(center=np.array((0.0, 0.0, -5.0)), radius=1.0, material=metal)), kat.ray7((0, 0, 0), (0, 0, -1)), 50),
           "mirrors": (kat.world_of(H.sphere(center=np.array((0.0, 0.0, -1001.0)), radius=1000.0, material=mirror),
                                    H.sphere(center=np.array((0.0, 0.0, 1001.0)), radius=1000.0, material=mirror)), kat.ray7((0, 0, 0), (0, 0, 1)), 50),
           "k15-furnace": (kat.world_of(H.sphere(center=np.zeros(3), radius=1000.0, material=light), H.sphere(center=np.array((0.0, 0.0, -5.0)), radius=1.0, material=lam)),
                           kat.ray7((0, 0, 0), (0, 0, -1)), 50)}
    for name, (w, ray, depth) in k13.items():
        rays = np.tile(np.asarray(ray, np.float64), (N_PROBES, 1))
        out.append(OracleCall("probe_paths", "oracle/kat/k13/" + name, w, n=N_PROBES, rays=rays.reshape(-1), keys=np.arange(N_PROBES, dtype=np.uint64) + 100, ctr0=0,
                              depth=depth, max_seg=52))
    return out


def oracle_expected_line(oracle, c):
    """the line oracle/san_main.c prints for call c, from what the ordinary librt_oracle.so returns through oracle.py"""
    s, n, a = "%s %s" % (c.label, c.kind), c.num("n"), c.args
    if c.kind == "render":
        lin, q, cnt = oracle.render(c.fs, c.num("nx"), c.num("ny"), c.num("ns"), c.num("depth"), c.num("seed"), nthreads=c.num("nthreads"))
        return s + " rc=0" + _hex("linear", fnv1a(lin.tobytes())) + _hex("rgb8", fnv1a(q.tobytes())) + " counters=%d,%d" % (int(cnt[0]), int(cnt[1]))
    if c.kind == "probe_hit":
        return s + _hash("hits", oracle.probe_hit(c.fs, a["rays"], float(a["tmin"][0]), float(a["tmax"][0]), bvh_seed=a.get("bvh_seed")))
    if c.kind == "probe_paths":
        rgb, nseg, log, nlog = oracle.probe_paths(c.fs, a["rays"], a["keys"], depth=c.num("depth"), ctr0=c.num("ctr0"), max_seg=c.num("max_seg"))
        return s + _hash("rgb", rgb) + _hash("nseg", nseg) + _hash("nlog", nlog) + (_hash("log", log) if log is not None else "")
    if c.kind == "probe_camera":
        return s + _hash("rays", oracle.probe_camera(c.fs, a["uv"], a["keys"]))
    if c.kind == "probe_texture":
        return s + _hash("rgb", oracle.probe_texture(c.fs, c.num("tex"), a["uvp"]))
    if c.kind == "probe_scatter":
        return s + _hash("out", oracle.probe_scatter(c.fs, c.num("mat"), a["rays"], a["hits"], a["keys"]))
    raise ValueError(c.kind)
