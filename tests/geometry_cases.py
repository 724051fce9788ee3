"""Scenes, edits and references for the tests of rtmi_scene_set_geometry (test_geometry_host.py on the CPU, test_gpu_geometry.py on the device).
Host records and numpy only, plus the library's host-only hooks: nothing here touches a device.

An EDIT is a copy of a FlatScene with other prim_geom / xform_param (`edited`).  `refit` runs the host hook rtmi_test_refit over a sequence of
FlatScenes with one structure; `numpy_refit` recomputes a node array bottom-up, independently of the library."""
import copy

import numpy as np

import raytrace_clj_amd as r
from raytrace_clj_amd import _ffi
from raytrace_clj_amd import flatten as fl

BVH_EMPTY = -0x80000000
NX, NY, NS = 36, 20, 4
COVER_N = 9  # make_random_scene(..., 9, ...): 326 primitives, 322 of them in the layer -- an entry grid is built (>= 256)


def cover(moving=False):
    return fl.flatten(r.scene.make_random_scene(NX, NY, COVER_N, moving))


def edited(flat, change):
    """a copy of `flat` whose prim_geom and xform_param `change(prim_geom, xform_param)` has altered in place"""
    f = copy.copy(flat)
    f.prim_geom = np.array(flat.prim_geom, np.float64, copy=True)
    f.xform_param = np.array(flat.xform_param, np.float64, copy=True).reshape(-1, 3)
    change(f.prim_geom, f.xform_param)
    return f


def kinds(flat):
    return np.asarray(flat.prim_kind, np.int32) & ~fl.PRIM_BOUNDARY


def small_spheres(flat, r_max=0.5):
    """indices of the plain spheres of the cover scene's layer"""
    k, g = kinds(flat), np.asarray(flat.prim_geom)
    return np.flatnonzero((k <= fl.PRIM_MOVING) & (np.abs(g[:, 3]) < r_max))


def shrink_and_nudge(flat, which, step=1e-3, factor=0.9):
    """spheres `which`: radius times `factor`, centre moved by `step` along x and z (alternating signs): each new box lies inside the old one as long as
    (1 - factor) r > step, so nothing leaves its cells or the trees' bounds"""
    def change(g, xp):
        for n, i in enumerate(which):
            g[i, 0] += step * (1 if n % 2 else -1)
            g[i, 2] += step * (1 if n % 3 else -1)
            g[i, 3] *= factor
            if kinds(flat)[i] == fl.PRIM_MOVING:
                g[i, 4] += step * (1 if n % 2 else -1)
                g[i, 6] += step * (1 if n % 3 else -1)
    return edited(flat, change)


def refit(steps, want_nodes=True):
    """rtmi_test_refit over FlatScenes of one structure -> dict(rc, nodes (bytes as uint8), node16, root, tall, grid_n, n_big, displaced, rebuilt, records,
    launches, rebuilds, big (list), cells, leaf_box [n_world, 6] float32)"""
    f0 = steps[0]
    a = lambda x, dt: np.ascontiguousarray(x, dt)
    n = len(f0.prim_kind)
    pk, flip, xf = a(f0.prim_kind, np.int32), a(f0.prim_flip, np.int32), a(f0.prim_xform, np.int32)
    xk, cam = a(f0.xform_kind, np.int32), a(f0.cam, np.float64)
    geoms = a(np.stack([np.asarray(f.prim_geom, np.float64).reshape(n, -1) for f in steps]), np.float64)
    xforms = a(np.stack([np.asarray(f.xform_param, np.float64).reshape(-1, 3) for f in steps]), np.float64) if len(xk) else None
    p = _ffi.ptr
    L = _ffi.lib()
    nbytes, info, big = np.zeros(1, np.int64), np.zeros(10, np.int32), np.zeros(16, np.int32)
    args = (n, p(pk), p(flip), p(xf), len(xk), p(xk) if len(xk) else None, int(f0.cam_kind), p(cam), len(steps), p(geoms), p(xforms))
    rc = L.rtmi_test_refit(*args, None, 0, p(nbytes), p(info), p(big), None, 0, None)
    out = {"rc": rc}
    if rc:
        out["error"] = L.rtmi_last_error().decode()
        return out
    nodes = np.zeros(max(int(nbytes[0]), 1), np.uint8)
    g = int(info[3])
    cells = np.zeros(max(4 * g * g, 1), np.int32)
    n_world = int(np.count_nonzero((pk & fl.PRIM_BOUNDARY) == 0))
    leaf_box = np.zeros((max(n_world, 1), 6), np.float32)
    if want_nodes:
        rc = L.rtmi_test_refit(*args, p(nodes), len(nodes), p(nbytes), p(info), p(big), p(cells), len(cells), p(leaf_box))
        assert rc == 0
    keys = ("node16", "root", "tall", "grid_n", "n_big", "displaced", "rebuilt", "records", "launches", "rebuilds")
    out.update({k: int(v) for k, v in zip(keys, info)})
    out.update(nodes=nodes[:int(nbytes[0])], big=[int(v) for v in big[:int(info[4])]], cells=cells[:4 * g * g], leaf_box=leaf_box[:n_world])
    return out


def child_codes(nodes, node16):
    """[n_nodes, 2] int32 child codes of a node array (uint8 bytes)"""
    if node16:
        return nodes.view(np.int32).reshape(-1, 8)[:, 6:8]
    return nodes.view(np.int32).reshape(-1, 16)[:, 12:14]


def _half_outward(x, up):
    """float32 array -> the float16 at or beyond it (numpy's own rounding, corrected outward)"""
    with np.errstate(over="ignore"):
        h = x.astype(np.float16)
    wrong = (h.astype(np.float32) < x) if up else (h.astype(np.float32) > x)
    moved = np.nextafter(h, np.float16(np.inf if up else -np.inf))
    return np.where(wrong, moved, h)


def numpy_refit(nodes, node16, leaf_box):
    """The node array recomputed bottom-up from leaf_box alone: records by descending index (children lie behind their parents), a box = the
    leaf's box (through the outward half rounding for half records), the empty box (no child, or the right side of a lone primitive's node,
    which names its leaf on both sides), or the union of the child record's two boxes.  Returns the
    planes as [n_nodes, 2 sides, 2 (lo, hi), 3] and the same view of the array given, for np.array_equal."""
    codes = child_codes(nodes, node16)
    n = len(codes)
    if node16:
        p = nodes.view(np.float16).reshape(n, 16)[:, :12].reshape(n, 2, 3, 2)  # side, axis, (lo, hi)
        have = np.transpose(p, (0, 1, 3, 2)).copy()
        lb_lo, lb_hi = _half_outward(leaf_box[:, :3], False), _half_outward(leaf_box[:, 3:], True)
        dt, rec = np.float16, 32
    else:
        q = nodes.view(np.float32).reshape(n, 16)
        have = np.zeros((n, 2, 2, 3), np.float32)
        for s in range(2):
            have[:, s, 0, 0], have[:, s, 0, 1], have[:, s, 0, 2] = q[:, s * 4], q[:, s * 4 + 1], q[:, 8 + s * 2]
            have[:, s, 1, 0], have[:, s, 1, 1], have[:, s, 1, 2] = q[:, s * 4 + 2], q[:, s * 4 + 3], q[:, 8 + s * 2 + 1]
        lb_lo, lb_hi = leaf_box[:, :3], leaf_box[:, 3:]
        dt, rec = np.float32, 64
    want = np.zeros((n, 2, 2, 3), dt)
    for k in range(n - 1, -1, -1):
        for s in range(2):
            c = int(codes[k, s])
            if c == BVH_EMPTY or (s == 1 and c < 0 and c == int(codes[k, 0])):  # (a lone primitive's node names its leaf twice: the right box is empty)
                want[k, s, 0], want[k, s, 1] = np.inf, -np.inf
            elif c < 0:
                i = ~c & 0x1fffffff
                want[k, s, 0], want[k, s, 1] = lb_lo[i], lb_hi[i]
            else:
                ch = c // rec
                assert c % rec == 0 and k < ch < n
                want[k, s, 0] = np.minimum(want[ch, 0, 0], want[ch, 1, 0])
                want[k, s, 1] = np.maximum(want[ch, 0, 1], want[ch, 1, 1])
    return want, have


def pack_geometry_hash(flat, through_creation):
    a = lambda x, dt: np.ascontiguousarray(x, dt)
    pk, pg, pm = a(flat.prim_kind, np.int32), a(flat.prim_geom, np.float64), a(flat.prim_mat, np.int32)
    mk, mt, mp = a(flat.mat_kind, np.int32), a(flat.mat_tex, np.int32), a(flat.mat_param, np.float64)
    tk, tp, tc = a(flat.tex_kind, np.int32), a(flat.tex_param, np.float64), a(flat.tex_child, np.int32)
    c24, flip, xf = a(flat.cam, np.float64), a(flat.prim_flip, np.int32), a(flat.prim_xform, np.int32)
    xk, xp = a(flat.xform_kind, np.int32), a(flat.xform_param, np.float64)
    h = np.zeros(1, np.uint64)
    p = _ffi.ptr
    rc = _ffi.lib().rtmi_test_pack_geometry(len(pk), p(pk), p(pg), p(pm), len(mk), p(mk), p(mt), p(mp), len(tk), p(tk), p(tp), p(tc), int(flat.cam_kind), p(c24),
                                            p(flip), p(xf), len(xk), p(xk), p(xp) if len(xk) else None, int(through_creation), p(h))
    return rc, int(h[0])
