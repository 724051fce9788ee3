"""Host mirror of raytrace-clj.core (src/raytrace_clj/core.clj): the driver.

`render` replaces the render loop of -main (core.clj:100-108): instead of cp/upmap over 32-pixel
chunks calling `pixel` (core.clj:43-57) -> `color` (core.clj:17-41) on the JVM, the scene is flattened
once (flatten.py) and the whole loop runs in the HIP kernels behind librtmi.so.  `main` keeps the
reference's positional CLI `name nx ny ns` (core.clj:73-80) and the progress/summary line
(display.clj:20-24); the cover scene (core.clj:89) is the default scene.

hit / scatter / emitted / sample / get_ray are the protocol entry points (hitable.clj:7-10,
shader.clj:22-24, texture.clj:8-9, camera.clj:5-6): each runs the SAME device function the render
kernel uses, for one call, through the probe entry points of the C-ABI.  Nothing here computes on the CPU."""
import copy
import ctypes as C
import sys
import time

import numpy as np

from . import _ffi
from . import camera as cam
from . import flatten as fl
from . import hitable as hitm
from . import shader as shad
from . import texture as texm
from ._ffi import F32, F64, RtmiError, check, ptr

T_MIN = 0.001
T_MAX = 3.4028234663852886e38  # Float/MAX_VALUE, core.clj:25
DEFAULT_DEPTH = 50              # core.clj:20,45
RENDER_SEED = 0x5EED0002

# the denoiser's defaults: chosen by a grid over the small cover scene and the Cornell box at 16 spp
DENOISE_ITERATIONS = 5
DENOISE_SIGMA_C = 4.0
DENOISE_SIGMA_N = 0.5
DENOISE_SIGMA_A = 0.2
DENOISE_SIGMA_D = 0.2
FEATURE_SAMPLES = 4

# temporal accumulation's defaults: chosen by a grid over the Cornell box and the small cover scene at 4 spp per view
REPROJECT_MAX_HISTORY = 8.0
REPROJECT_SIGMA_D = 0.1
REPROJECT_SIGMA_N = 0.0
REPROJECT_SIGMA_A = 0.0

_PRECISION = {"f64": F64, "f32": F32, F64: F64, F32: F32}


class Context:
    """One rtmi_ctx: a HIP device binding (one per process/GPU)."""

    def __init__(self, device=0, timing=False):
        L = _ffi.lib()
        h = C.c_void_p()
        check(L.rtmi_init(int(device), _ffi.FLAG_TIMING if timing else 0, C.byref(h)))
        self.handle = h
        self.device = int(device)

    def set_option(self, name, value):
        check(_ffi.lib().rtmi_set_option(self.handle, name.encode(), int(value)))

    def device_info(self):
        cus, lds, hbm = C.c_int32(), C.c_int32(), C.c_int64()
        arch = C.create_string_buffer(64)
        check(_ffi.lib().rtmi_device_info(self.handle, C.byref(cus), C.byref(lds), C.byref(hbm), arch, 64))
        return {"compute_units": cus.value, "lds_bytes_per_cu": lds.value, "hbm_bytes": hbm.value, "arch": arch.value.decode()}

    def last_trace_ms(self):
        ms, n = C.c_double(), C.c_int32()
        check(_ffi.lib().rtmi_last_trace_ms(self.handle, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def last_accel(self):
        """'bvh' or 'flat': what the last render ran (a small mixed-kind scene is scanned even when the tree was asked for: option flat_below)"""
        v = C.c_int32()
        check(_ffi.lib().rtmi_last_accel(self.handle, C.byref(v)))
        return "bvh" if v.value == _ffi.ACCEL_BVH else "flat"

    def last_reduce_ms(self):
        """(sum of reduce_kernel ms, launches) of the window the last last_trace_ms() call closed"""
        ms, n = C.c_double(), C.c_int32()
        check(_ffi.lib().rtmi_last_reduce_ms(self.handle, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def progressive_samples(self):
        """k of the context's progressive frame (samples [0, k) it holds), 0 = none"""
        k = C.c_int32()
        check(_ffi.lib().rtmi_progressive_samples(self.handle, C.byref(k)))
        return k.value

    def progressive_release(self):
        """drop the context's progressive frame and free its buffers"""
        check(_ffi.lib().rtmi_progressive_release(self.handle))

    def adaptive_status(self):
        """(tiles still active, local tiles of the frame, sum over the region's pixels of the samples their tile holds) of the context's
        progressive frame; zeros without one.  Host state only."""
        a, t, n = C.c_int32(), C.c_int32(), C.c_int64()
        check(_ffi.lib().rtmi_adaptive_status(self.handle, C.byref(a), C.byref(t), C.byref(n)))
        return a.value, t.value, n.value

    def adaptive_active_tiles(self):
        """global tile indices (row-major over the 8x8 tiles of the frame) of the tiles still active, int32, ascending"""
        n = C.c_int32()
        check(_ffi.lib().rtmi_adaptive_active_tiles(self.handle, 0, None, C.byref(n)))
        out = np.zeros(n.value, np.int32)
        if n.value:
            check(_ffi.lib().rtmi_adaptive_active_tiles(self.handle, n.value, ptr(out), C.byref(n)))
        return out

    def adaptive_retire(self, noise, eps):
        """Retire the active tiles of the context's progressive frame whose pixels inside the frame's region all pass noise <= eps (a NaN
        fails) -> the number of tiles this call retired.  noise: [ny, nx] float64 of the WHOLE frame, row 0 = top -- denoise's stderr as it
        is.  No samples are added; the frame's sums, sample counts and counters stay as they are."""
        m = np.ascontiguousarray(noise, np.float64)
        if m.ndim != 2:
            raise ValueError("noise must be [ny, nx]")
        n = C.c_int32()
        check(_ffi.lib().rtmi_adaptive_retire(self.handle, m.shape[1], m.shape[0], ptr(m), float(eps), C.byref(n)))
        return n.value

    def assemble_progressive_device(self, nx, ny, world, tiles_per_rank, gathered_rec, out_linear=None, out_rgb8=None, out_stderr=None,
                                    out_samples=None, stream=None):
        """gathered tile records [world, tiles_per_rank, 64, 5] (rank r's k-th tile is global tile r + k * world) -> the dense frame: linear,
        rgb8, stderr [ny, nx] float64, samples [ny, nx] int32, HBM-resident, each may be None; asynchronous, render_device's stream semantics"""
        check(_ffi.lib().rtmi_assemble_progressive_device(self.handle, nx, ny, world, tiles_per_rank, ptr(gathered_rec), ptr(out_linear),
                                                          ptr(out_rgb8), ptr(out_stderr), ptr(out_samples), ptr(stream)))

    def adaptive_retire_device(self, nx, ny, noise, eps, stream=None):
        """adaptive_retire on an HBM-resident map (a torch tensor or a raw device pointer; render_device's stream semantics; synchronises the
        stream once, at the end of the call: the host reads the number of tiles still active) -> the number of tiles retired"""
        n = C.c_int32()
        check(_ffi.lib().rtmi_adaptive_retire_device(self.handle, nx, ny, ptr(noise), float(eps), C.byref(n), ptr(stream)))
        return n.value

    def tiles_retire(self, noise, eps, tiles):
        """The stateless adaptive_retire (rtmi_tiles_retire): of the listed 8x8 tiles (global indices, row-major over the frame's tiles) those
        with a pixel inside the image that fails noise <= eps (NaN and +inf fail), in the list's order -> int32 array.  noise: [ny, nx] float64
        of the whole frame -- render_lit_tiles' stderr or denoise's as it is.  No frame of the context is read or changed."""
        m = np.ascontiguousarray(noise, np.float64)
        if m.ndim != 2:
            raise ValueError("noise must be [ny, nx]")
        tiles = np.ascontiguousarray(tiles, np.int32).reshape(-1)
        out, n = np.zeros(max(len(tiles), 1), np.int32), C.c_int32()
        check(_ffi.lib().rtmi_tiles_retire(self.handle, m.shape[1], m.shape[0], ptr(m), float(eps), len(tiles), ptr(tiles), ptr(out), C.byref(n)))
        return out[:n.value].copy()

    def tiles_retire_device(self, nx, ny, noise, eps, n_tiles, tiles_in, tiles_out=None, stream=None):
        """tiles_retire on HBM-resident buffers (torch tensors or raw device pointers; render_device's stream semantics; synchronises the stream
        once: the host reads the number of survivors) -> that number; the survivors are the first entries of tiles_out (None: of tiles_in itself)"""
        n = C.c_int32()
        check(_ffi.lib().rtmi_tiles_retire_device(self.handle, int(nx), int(ny), ptr(noise), float(eps), int(n_tiles), ptr(tiles_in),
                                                  ptr(tiles_in if tiles_out is None else tiles_out), C.byref(n), ptr(stream)))
        return n.value

    def lit_tiles_records_device(self, nx, ny, tile_first, tile_stride, n_slots, state, linear, stderr, out_rec, stream=None):
        """rtmi_lit_tiles_records_device: the dealt tiles tile_first, tile_first + tile_stride, ... out of render_lit_tiles_device's whole-frame
        buffers (state [nx * ny, RAYS_REC], linear [ny, nx, 3], stderr [ny, nx]) into out_rec [n_slots, 64, PROG_REC] -- mean, stderr, samples per
        pixel, the record assemble_progressive_device takes; pixels outside the image and slots past the last tile are zeros.  HBM-resident
        buffers; asynchronous, render_device's stream semantics."""
        check(_ffi.lib().rtmi_lit_tiles_records_device(self.handle, int(nx), int(ny), int(tile_first), int(tile_stride), int(n_slots), ptr(state),
                                                       ptr(linear), ptr(stderr), ptr(out_rec), ptr(stream)))

    # ---- the edge-aware denoiser: a pure image operation (rtmi_denoise*) ---------------------------------------------------------
    def denoise(self, linear, stderr=None, features=None, iterations=DENOISE_ITERATIONS, sigma_c=DENOISE_SIGMA_C, sigma_n=DENOISE_SIGMA_N,
                sigma_a=DENOISE_SIGMA_A, sigma_d=DENOISE_SIGMA_D):
        """A-trous wavelet filter of a frame [h,w,3] guided by its standard error [h,w] (render_progressive / render_adaptive) and its feature
        buffers [h,w,8] (render_features), either of which may be None -> (linear, rgb8, stderr) after `iterations` passes.  A sigma of 0
        switches its term off; iterations = 0 returns the input."""
        lin = np.ascontiguousarray(linear, np.float64)
        if lin.ndim != 3 or lin.shape[2] != 3:
            raise ValueError("linear must be [h, w, 3]")
        h, w = lin.shape[:2]
        se = None if stderr is None else np.ascontiguousarray(stderr, np.float64)
        ft = None if features is None else np.ascontiguousarray(features, np.float64)
        if se is not None and se.shape != (h, w):
            raise ValueError("stderr must be [h, w]")
        if ft is not None and ft.shape != (h, w, _ffi.FEATURES):
            raise ValueError("features must be [h, w, %d]" % _ffi.FEATURES)
        out, q, err = np.zeros_like(lin), np.zeros(lin.shape, np.uint8), np.zeros((h, w), np.float64)
        check(_ffi.lib().rtmi_denoise(self.handle, w, h, ptr(lin), ptr(se), ptr(ft), int(iterations), float(sigma_c), float(sigma_n),
                                      float(sigma_a), float(sigma_d), ptr(out), ptr(q), ptr(err)))
        return out, q, err

    def denoise_device(self, nx, ny, linear, stderr=None, features=None, out_linear=None, out_rgb8=None, out_stderr=None,
                       iterations=DENOISE_ITERATIONS, sigma_c=DENOISE_SIGMA_C, sigma_n=DENOISE_SIGMA_N, sigma_a=DENOISE_SIGMA_A,
                       sigma_d=DENOISE_SIGMA_D, stream=None):
        """denoise on HBM-resident buffers (torch tensors or raw device pointers), asynchronous, render_device's stream semantics"""
        check(_ffi.lib().rtmi_denoise_device(self.handle, nx, ny, ptr(linear), ptr(stderr), ptr(features), int(iterations), float(sigma_c),
                                             float(sigma_n), float(sigma_a), float(sigma_d), ptr(out_linear), ptr(out_rgb8), ptr(out_stderr),
                                             ptr(stream)))

    # ---- temporal accumulation: the previous frame reprojected into a moved camera (rtmi_reproject*) -------------------------------------
    def reproject(self, prev_camera, cur_camera, prev_linear, prev_weight, prev_stderr, prev_features, cur_linear, cur_stderr, cur_features,
                  cur_weight, max_history=REPROJECT_MAX_HISTORY, sigma_d=REPROJECT_SIGMA_D, sigma_n=REPROJECT_SIGMA_N, sigma_a=REPROJECT_SIGMA_A):
        """Blend a history (colour [h,w,3], accumulated samples [h,w], standard error [h,w] or None, the features [h,w,8] and the camera it was
        seen with) into the current frame (colour, standard error or None, features, camera, its samples cur_weight): every pixel whose world
        point is found in the history -- same surface by depth / normal / albedo within the sigmas, 0 = test off -- becomes the weighted mean of
        both, the history's weight capped at max_history -> (linear, rgb8, weight, stderr or None, counters {pixels, pixels that took history}).
        Cameras: Camera records or (cam_kind, cam24) pairs."""
        (pk, pc), (ck, cc) = _camera_pair(prev_camera), _camera_pair(cur_camera)
        cl = np.ascontiguousarray(cur_linear, np.float64)
        if cl.ndim != 3 or cl.shape[2] != 3:
            raise ValueError("cur_linear must be [h, w, 3]")
        h, w = cl.shape[:2]
        shapes = {"prev_linear": (h, w, 3), "prev_weight": (h, w), "prev_stderr": (h, w), "prev_features": (h, w, _ffi.FEATURES),
                  "cur_stderr": (h, w), "cur_features": (h, w, _ffi.FEATURES)}
        given = {"prev_linear": prev_linear, "prev_weight": prev_weight, "prev_stderr": prev_stderr, "prev_features": prev_features,
                 "cur_stderr": cur_stderr, "cur_features": cur_features}
        a = {}
        for name, v in given.items():
            a[name] = None if v is None else np.ascontiguousarray(v, np.float64)
            if a[name] is not None and a[name].shape != shapes[name]:
                raise ValueError("%s must be %s" % (name, list(shapes[name])))
        both = a["prev_stderr"] is not None and a["cur_stderr"] is not None
        out, q, wt = np.zeros_like(cl), np.zeros(cl.shape, np.uint8), np.zeros((h, w), np.float64)
        err = np.zeros((h, w), np.float64) if both else None
        cnt = np.zeros(2, np.uint64)
        check(_ffi.lib().rtmi_reproject(self.handle, w, h, pk, ptr(pc), ck, ptr(cc), ptr(a["prev_linear"]), ptr(a["prev_weight"]),
                                        ptr(a["prev_stderr"]), ptr(a["prev_features"]), ptr(cl), ptr(a["cur_stderr"]), ptr(a["cur_features"]),
                                        float(cur_weight), float(max_history), float(sigma_d), float(sigma_n), float(sigma_a),
                                        ptr(out), ptr(q), ptr(wt), ptr(err), ptr(cnt)))
        return out, q, wt, err, cnt

    def reproject_device(self, nx, ny, prev_camera, cur_camera, prev_linear, prev_weight, prev_stderr, prev_features, cur_linear, cur_stderr,
                         cur_features, cur_weight, out_linear=None, out_rgb8=None, out_weight=None, out_stderr=None, out_counters=None,
                         max_history=REPROJECT_MAX_HISTORY, sigma_d=REPROJECT_SIGMA_D, sigma_n=REPROJECT_SIGMA_N, sigma_a=REPROJECT_SIGMA_A,
                         stream=None):
        """reproject on HBM-resident buffers (torch tensors or raw device pointers), asynchronous, render_device's stream semantics; the cameras
        stay host values.  Outputs may alias the cur_* buffers, never the prev_* ones."""
        (pk, pc), (ck, cc) = _camera_pair(prev_camera), _camera_pair(cur_camera)
        check(_ffi.lib().rtmi_reproject_device(self.handle, nx, ny, pk, ptr(pc), ck, ptr(cc), ptr(prev_linear), ptr(prev_weight), ptr(prev_stderr),
                                               ptr(prev_features), ptr(cur_linear), ptr(cur_stderr), ptr(cur_features), float(cur_weight),
                                               float(max_history), float(sigma_d), float(sigma_n), float(sigma_a), ptr(out_linear), ptr(out_rgb8),
                                               ptr(out_weight), ptr(out_stderr), ptr(out_counters), ptr(stream)))

    def last_traversal_counters(self):
        """(AABB slab tests, exact primitive tests) of the last render; needs set_option("count_traversal", 1) before it
        (metrics.clj:10 aabb.intersection.total, for the device's own tree)"""
        a, b = C.c_uint64(), C.c_uint64()
        check(_ffi.lib().rtmi_last_traversal_counters(self.handle, C.byref(a), C.byref(b)))
        return a.value, b.value

    def close(self):
        if self.handle:
            _ffi.lib().rtmi_shutdown(self.handle)
            self.handle = None


def _camera_pair(camera):
    """a Camera record or a (cam_kind, cam24) pair -> (int kind, float64 [24])"""
    kind, c = camera if isinstance(camera, tuple) else fl.flatten_camera(camera)
    c = np.ascontiguousarray(c, np.float64)
    if c.shape != (24,):
        raise ValueError("cam must hold 24 doubles")
    return int(kind), c


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


MATERIAL_FIELDS = ("mat_kind", "mat_tex", "mat_param", "tex_kind", "tex_param", "tex_child", "prim_mat")  # what set_materials replaces


def scene_arrays(f, **edit):
    """A FlatScene as rtmi.h's SceneArrays -> (arrays, args): the contiguous arrays by field name and the 19 C arguments made of them, n_prims
    first, xform_param last.  edit: arrays that stand in for the FlatScene's own (an edit, marshalled with the rest of the scene it applies to).
    A scene without the instancing arrays -- one assembled by hand, or with them at another length -- gets "no flips, no instances".
    `arrays` owns the memory `args` points into: keep it while the arguments are in use."""
    def field(name, dt, *default):
        return np.ascontiguousarray(edit[name] if name in edit else getattr(f, name, *default), dt)
    a = {name: field(name, dt) for name, dt in (
        ("prim_kind", np.int32), ("prim_geom", np.float64), ("prim_mat", np.int32), ("mat_kind", np.int32), ("mat_tex", np.int32),
        ("mat_param", np.float64), ("tex_kind", np.int32), ("tex_param", np.float64), ("tex_child", np.int32), ("cam", np.float64))}
    n = len(a["prim_kind"])
    for name, dt, shape in (("prim_flip", np.int32, n), ("prim_xform", np.int32, (n, 2)), ("xform_kind", np.int32, 0), ("xform_param", np.float64, (0, 3))):
        a[name] = field(name, dt, np.zeros(shape))
    if len(a["prim_flip"]) != n or len(a["prim_xform"]) != n:
        a["prim_flip"], a["prim_xform"] = np.zeros(n, np.int32), np.zeros((n, 2), np.int32)
    p = {name: ptr(v) for name, v in a.items()}
    args = (n, p["prim_kind"], p["prim_geom"], p["prim_mat"], len(a["mat_kind"]), p["mat_kind"], p["mat_tex"], p["mat_param"],
            len(a["tex_kind"]), p["tex_kind"], p["tex_param"], p["tex_child"], int(f.cam_kind), p["cam"],
            p["prim_flip"], p["prim_xform"], len(a["xform_kind"]), p["xform_kind"], p["xform_param"])
    return a, args


class DeviceScene:
    """A flattened scene resident in HBM (rtmi_scene)."""

    def __init__(self, scene, camera=None, ctx=None):
        self.ctx = ctx or default_context()
        self.flat = scene if isinstance(scene, fl.FlatScene) else fl.flatten(scene, camera)
        f = self.flat
        h = C.c_void_p()
        keep, args = scene_arrays(f)
        check(_ffi.lib().rtmi_scene_create_ex(self.ctx.handle, *args, C.byref(h)))
        self.handle = h
        if getattr(f, "perlin_vectors", None) is not None:  # perlin.clj:6-17 tables (seeded)
            vec = np.ascontiguousarray(f.perlin_vectors, np.float64)
            perm = np.ascontiguousarray(f.perlin_perm, np.int32)
            check(_ffi.lib().rtmi_scene_set_perlin(h, ptr(vec), ptr(perm)))
        calls = getattr(f, "media_calls", None)
        if calls is not None and len(calls) and getattr(f, "media_mode", 0) == 2:  # Hitlists holding media below bvh-nodes: the call sequence with its narrowing ranges
            calls = np.ascontiguousarray(calls, np.int32)
            lo = np.ascontiguousarray(f.media_narrow_from, np.int32)
            check(_ffi.lib().rtmi_scene_set_media_calls_narrowed(h, len(calls), ptr(calls), ptr(lo)))
        elif calls is not None and len(calls):  # ConstantMedium hit? invocation order (a medium in a one-item bvh leaf is asked twice)
            calls = np.ascontiguousarray(calls, np.int32)
            check(_ffi.lib().rtmi_scene_set_media_calls(h, len(calls), ptr(calls)))
        if getattr(f, "media_mode", 0) == 1:  # the world is a Hitlist holding media: their hit? sees the t-max narrowed by the items before them
            check(_ffi.lib().rtmi_scene_set_media_mode(h, int(f.media_mode)))
        images = getattr(f, "images", None) or []
        if images:  # ImageMap pixels (texture.clj:126-133)
            imgs = [np.ascontiguousarray(im, np.uint8) for im in images]
            wh = np.ascontiguousarray([[im.shape[1], im.shape[0]] for im in imgs], np.int32)
            rgb = np.ascontiguousarray(np.concatenate([im.reshape(-1) for im in imgs]), np.uint8)
            check(_ffi.lib().rtmi_scene_set_images(h, len(imgs), ptr(wh), ptr(rgb)))

    def clone(self, ctx):
        """the same scene replicated onto another context / device (rtmi_scene_clone)"""
        h = C.c_void_p()
        check(_ffi.lib().rtmi_scene_clone(self.handle, ctx.handle, C.byref(h)))
        other = object.__new__(DeviceScene)
        other.ctx, other.flat, other.handle = ctx, self.flat, h
        return other

    def close(self):
        if self.handle:
            _ffi.lib().rtmi_scene_destroy(self.handle)
            self.handle = None

    # ---- the camera of the live scene (rtmi_scene_set_camera*): another viewpoint or shutter without a new scene -------------------------
    def set_camera(self, camera, stream=None):
        """Give the live scene another camera: a Camera record or a (cam_kind, cam24) pair -> rebuilt (bool).  Every render afterwards equals,
        bit for bit, the render of a scene created fresh with that camera.  stream=None: the host form -- it waits for the context's stream,
        and if the scene holds MovingSpheres and the camera's shutter interval lies outside the one the scene was built for it rebuilds the
        trees (True).  With a stream (a hipStream_t handle or torch stream; 0 = the context's own) the camera travels in stream order and the
        host is never waited for: renders queued before it keep the old camera; a shutter that does not fit raises RtmiError -3."""
        kind, c = camera if isinstance(camera, tuple) else fl.flatten_camera(camera)
        c = np.ascontiguousarray(c, np.float64)
        if c.shape != (24,):
            raise ValueError("cam must hold 24 doubles")
        if stream is not None:
            handle = getattr(stream, "cuda_stream", stream)
            check(_ffi.lib().rtmi_scene_set_camera_stream(self.handle, int(kind), ptr(c), ptr(int(handle)) if handle else None))
            return False
        rebuilt = C.c_int32()
        check(_ffi.lib().rtmi_scene_set_camera(self.handle, int(kind), ptr(c), C.byref(rebuilt)))
        return bool(rebuilt.value)

    # ---- the materials of the live scene (rtmi_scene_set_materials*): other surfaces without a new scene ------------------------------
    def set_materials(self, scene_or_flat, stream=None):
        """Give the live scene other materials and textures: a FlatScene, or a scene (flattened here; its camera is not read) with the same
        primitives -> rebuilt (bool).  Its material and texture tables and its prim_mat replace the scene's; geometry, instancing and camera stay.
        Every render afterwards equals, bit for bit, the render of a scene created fresh from the edited arrays.  An edit that keeps the material
        and texture counts and the scene's kernels (no first Perlin / ImageMap / Isotropic use in a scene of plain spheres, no last one removed)
        rewrites the tables where they lie (False); any other rebuilds the scene behind the same handle (True) -- a new Perlin texture or image
        then still needs its tables, as at creation (rtmi_scene_set_perlin / _images; rendering raises RtmiError -5 until then).
        With a stream (a hipStream_t handle or torch stream; 0 = the context's own) only the changed rows travel, in stream order, and the host
        is never waited for: renders queued before keep the old materials.  An edit that would rebuild, or more than
        _ffi.EDIT_STREAM_MAX_BYTES of changed rows, raises RtmiError -3 and changes nothing.  ValueError if the primitive count differs.
        self.flat is replaced by a copy that holds the new arrays (clones share the old one and keep it)."""
        f = scene_or_flat if isinstance(scene_or_flat, fl.FlatScene) else fl.flatten(scene_or_flat)
        if len(f.prim_mat) != len(self.flat.prim_kind):
            raise ValueError("the edit has %d primitives, the scene %d" % (len(f.prim_mat), len(self.flat.prim_kind)))
        a, all_args = scene_arrays(self.flat, **{name: getattr(f, name) for name in MATERIAL_FIELDS})
        args = (self.handle,) + all_args[4:12] + (all_args[3],)  # n_mats + 3 arrays, n_tex + 3 arrays, prim_mat
        rebuilt = C.c_int32()
        if stream is not None:
            handle = getattr(stream, "cuda_stream", stream)
            check(_ffi.lib().rtmi_scene_set_materials_stream(*args, ptr(int(handle)) if handle else None))
        else:
            check(_ffi.lib().rtmi_scene_set_materials(*args, C.byref(rebuilt)))
        flat = copy.copy(self.flat)
        for name in MATERIAL_FIELDS:
            setattr(flat, name, a[name].copy())
        flat.tex_param, flat.tex_child = flat.tex_param.reshape(-1, fl.TEX_STRIDE), flat.tex_child.reshape(-1, 2)
        self.flat = flat
        return bool(rebuilt.value)

    # ---- the geometry of the live scene (rtmi_scene_set_geometry): primitives moved without a new scene ----------------------------------
    def _geometry_arrays(self, scene_or_flat):
        """the edit's prim_geom and xform_param, after the structure checks: ValueError unless counts, kinds, flips and instance chains are the scene's"""
        f = scene_or_flat if isinstance(scene_or_flat, fl.FlatScene) else fl.flatten(scene_or_flat)
        g = self.flat
        if len(f.prim_kind) != len(g.prim_kind):
            raise ValueError("the edit has %d primitives, the scene %d: a changed count is a new scene" % (len(f.prim_kind), len(g.prim_kind)))
        xk_f, xk_g = np.asarray(getattr(f, "xform_kind", np.zeros(0)), np.int32), np.asarray(getattr(g, "xform_kind", np.zeros(0)), np.int32)
        if len(xk_f) != len(xk_g):
            raise ValueError("the edit has %d instance records, the scene %d: a changed count is a new scene" % (len(xk_f), len(xk_g)))
        n = len(g.prim_kind)
        for name, shape in (("prim_kind", (n,)), ("prim_flip", (n,)), ("prim_xform", (n, 2)), ("xform_kind", (len(xk_g),))):
            a = np.asarray(getattr(f, name, np.zeros(shape)), np.int32).reshape(shape)
            b = np.asarray(getattr(g, name, np.zeros(shape)), np.int32).reshape(shape)
            if not np.array_equal(a, b):
                raise ValueError("the edit's %s differs from the scene's: kinds, flips and instance structure are not editable (a new scene)" % name)
        pg = np.ascontiguousarray(f.prim_geom, np.float64).reshape(n, -1)
        xp = np.ascontiguousarray(getattr(f, "xform_param", np.zeros((0, 3))), np.float64).reshape(-1, 3)
        return pg, xp

    def set_geometry(self, scene_or_flat, mode="auto"):
        """Move the live scene's primitives: a FlatScene, or a scene (flattened here; its camera and materials are not read) with the same
        structure -> info = {"rebuilt", "displaced", "nodes_refit", "launches"}.  Its prim_geom and xform_param replace the scene's.  Every
        result afterwards (frames, features, probes, ray counter) equals, bit for bit, that of a scene created fresh from the edited arrays; the
        tree keeps its topology and is refit on the device, so the traversal counters and tree_info() may differ.  mode "auto": in place if
        the edit fits the built trees (see rtmi.h), else a rebuild behind the same handle; "rebuild": always a fresh tree.  A primitive that
        leaves the entry-grid cells it was built into is displaced into the list of primitives every ray tests first ("displaced": how many
        are there now); a rebuild brings them home.  ValueError, before the library is touched, if counts, kinds, flips or the instance
        structure differ.  self.flat is replaced by a copy that holds the new arrays (clones share the old one and keep it)."""
        if mode not in ("auto", "rebuild"):
            raise ValueError("mode must be 'auto' or 'rebuild'")
        pg, xp = self._geometry_arrays(scene_or_flat)
        info = np.zeros(4, np.int32)
        check(_ffi.lib().rtmi_scene_set_geometry(self.handle, len(pg), ptr(pg), len(xp), ptr(xp) if len(xp) else None, 1 if mode == "rebuild" else 0, ptr(info)))
        flat = copy.copy(self.flat)
        flat.prim_geom = pg.copy()
        if len(xp):
            flat.xform_param = xp.copy()
        self.flat = flat
        return {"rebuilt": bool(info[0]), "displaced": int(info[1]), "nodes_refit": int(info[2]), "launches": int(info[3])}

    def last_refit_ms(self):
        """device time of the refit launches of the last in-place set_geometry (a Context(timing=True); waits for them)"""
        ms = C.c_double()
        check(_ffi.lib().rtmi_scene_last_refit_ms(self.handle, C.byref(ms)))
        return ms.value

    def camera_info(self):
        """-> {"cam_kind", "cam" (24 doubles), "built_t_lo", "built_t_hi"}: the camera the scene renders with now and the shutter interval its
        trees were built for (a camera whose interval lies inside it never rebuilds).  Host state only."""
        kind, lo, hi = C.c_int32(), C.c_double(), C.c_double()
        c = np.zeros(24, np.float64)
        check(_ffi.lib().rtmi_scene_camera(self.handle, C.byref(kind), ptr(c), C.byref(lo), C.byref(hi)))
        return {"cam_kind": kind.value, "cam": c, "built_t_lo": lo.value, "built_t_hi": hi.value}

    def tree_info(self):
        """-> (node records, depth of the deepest leaf, entry-grid cells per side, big primitives kept out of the tree) of the device's tree as
        the scene was built with it: what the launch decisions are taken from.  Host state only."""
        info = np.zeros(4, np.int32)
        check(_ffi.lib().rtmi_scene_tree_info(self.handle, ptr(info)))
        return tuple(int(v) for v in info)

    def render_views(self, cameras, nx, ny, ns, depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", stream=None, out_rgb8=None):
        """One frame per camera, queued back to back: for every view the stream form of set_camera, then render_device into its slice of ONE
        [V, ny, nx, 3] float64 device tensor (out_rgb8: an optional [V, ny, nx, 3] uint8 device tensor for the 8-bit frames), and ONE
        synchronisation at the end -> the tensor.  stream=None: the context's own stream.  The scene keeps the last camera."""
        import torch
        cameras = list(cameras)
        dev = torch.device("cuda", self.ctx.device)
        out = torch.empty((len(cameras), ny, nx, 3), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)  # (the allocator may have zero-filled or recycled on torch's stream; nothing of torch's is queued after this)
        handle = 0 if stream is None else getattr(stream, "cuda_stream", stream)
        for k, camera in enumerate(cameras):
            self.set_camera(camera, stream=handle)
            self.render_device(nx, ny, ns, out[k], None if out_rgb8 is None else out_rgb8[k], None, depth, seed, precision, handle or None)
        torch.cuda.synchronize(dev)
        return out

    # ---- the hot path, host buffers (what the JNA host calls) ---------------------------------------
    def render(self, nx, ny, ns, depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", region=None):
        """-> (linear float64 [h,w,3] = per-pixel mean before sqrt, rgb8 uint8 [h,w,3], counters {total-rays,total-pixels})"""
        x0, y0, x1, y1 = region if region is not None else (0, 0, nx, ny)
        lin = np.zeros((max(y1 - y0, 0), max(x1 - x0, 0), 3), np.float64)
        q = np.zeros(lin.shape, np.uint8)
        cnt = np.zeros(2, np.uint64)
        check(_ffi.lib().rtmi_render(self.handle, nx, ny, ns, depth, seed, _PRECISION[precision], x0, y0, x1, y1,
                                     ptr(lin), ptr(q), ptr(cnt)))
        return lin, q, cnt

    # ---- the hot path, HBM-resident buffers (torch tensors or raw device pointers) --------------------
    def render_device(self, nx, ny, ns, out_linear=None, out_rgb8=None, out_counters=None, depth=DEFAULT_DEPTH,
                      seed=RENDER_SEED, precision="f64", stream=None):
        check(_ffi.lib().rtmi_render_device(self.handle, nx, ny, ns, depth, seed, _PRECISION[precision],
                                            ptr(out_linear), ptr(out_rgb8), ptr(out_counters), ptr(stream)))

    # ---- progressive rendering: the context's one progressive frame, refined over calls ---------------------------------
    def render_progressive(self, nx, ny, s_first, s_count, depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", region=None):
        """Add samples [s_first, s_first + s_count) to the context's progressive frame (s_first = 0 starts one) -> (linear, rgb8, stderr [h,w],
        counters) after k = s_first + s_count samples: linear, rgb8 and counters equal render(ns = k) bit for bit; stderr = per pixel the largest
        channel's standard error of the mean (inf at k = 1)."""
        x0, y0, x1, y1 = region if region is not None else (0, 0, nx, ny)
        lin = np.zeros((max(y1 - y0, 0), max(x1 - x0, 0), 3), np.float64)
        q = np.zeros(lin.shape, np.uint8)
        err = np.zeros(lin.shape[:2], np.float64)
        cnt = np.zeros(2, np.uint64)
        check(_ffi.lib().rtmi_render_progressive(self.handle, nx, ny, s_first, s_count, depth, seed, _PRECISION[precision], x0, y0, x1, y1,
                                                 ptr(lin), ptr(q), ptr(err), ptr(cnt)))
        return lin, q, err, cnt

    def render_progressive_device(self, nx, ny, s_first, s_count, out_linear=None, out_rgb8=None, out_stderr=None, out_counters=None,
                                  depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", stream=None):
        """render_progressive for the whole frame into HBM-resident buffers (asynchronous, render_device's stream semantics)"""
        check(_ffi.lib().rtmi_render_progressive_device(self.handle, nx, ny, s_first, s_count, depth, seed, _PRECISION[precision],
                                                        ptr(out_linear), ptr(out_rgb8), ptr(out_stderr), ptr(out_counters), ptr(stream)))

    def refine(self, nx, ny, ns, chunk, depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", region=None):
        """Render progressively in chunks of `chunk` samples up to ns: yields (k, linear, rgb8, stderr, counters) after every chunk.  The
        caller may stop early; the frame after k samples is render(ns = k)'s."""
        if chunk <= 0 or ns <= 0:
            raise ValueError("ns and chunk must be > 0")
        k = 0
        while k < ns:
            n = min(chunk, ns - k)
            lin, q, err, cnt = self.render_progressive(nx, ny, k, n, depth, seed, precision, region)
            k += n
            yield k, lin, q, err, cnt

    # ---- adaptive sampling: the frame's 8x8 tiles stop taking samples once their noise is below eps -----------------------------
    def render_adaptive(self, nx, ny, s_first, s_count, eps, depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", region=None):
        """Add samples [s_first, s_first + s_count) to the active tiles of the context's progressive frame, then retire every tile whose
        pixels all have a standard error <= eps after k = s_first + s_count >= 2 samples -> (linear, rgb8, stderr [h,w], samples int32 [h,w],
        counters).  A pixel whose tile holds n samples equals render(ns = n) there bit for bit; counters[0] = the segments traced so far."""
        x0, y0, x1, y1 = region if region is not None else (0, 0, nx, ny)
        lin = np.zeros((max(y1 - y0, 0), max(x1 - x0, 0), 3), np.float64)
        q = np.zeros(lin.shape, np.uint8)
        err = np.zeros(lin.shape[:2], np.float64)
        smp = np.zeros(lin.shape[:2], np.int32)
        cnt = np.zeros(2, np.uint64)
        check(_ffi.lib().rtmi_render_adaptive(self.handle, nx, ny, s_first, s_count, float(eps), depth, seed, _PRECISION[precision], x0, y0, x1, y1,
                                              ptr(lin), ptr(q), ptr(err), ptr(smp), ptr(cnt)))
        return lin, q, err, smp, cnt

    def render_adaptive_device(self, nx, ny, s_first, s_count, eps, out_linear=None, out_rgb8=None, out_stderr=None, out_samples=None,
                               out_counters=None, depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", stream=None):
        """render_adaptive for the whole frame into HBM-resident buffers (render_device's stream semantics; synchronises the stream once, at the
        end of the call: the host reads the number of tiles still active)"""
        check(_ffi.lib().rtmi_render_adaptive_device(self.handle, nx, ny, s_first, s_count, float(eps), depth, seed, _PRECISION[precision],
                                                     ptr(out_linear), ptr(out_rgb8), ptr(out_stderr), ptr(out_samples), ptr(out_counters), ptr(stream)))

    def refine_adaptive(self, nx, ny, ns, chunk, eps, first=None, depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", region=None):
        """Render adaptively up to ns samples per pixel: a first round of `first` samples (default: chunk; the guard against retiring a tile on
        two lucky samples), then rounds of `chunk`; yields (k, linear, rgb8, stderr, samples, counters, active tiles) after every round and ends
        when no tile is active or k reaches ns."""
        first = chunk if first is None else first
        if chunk <= 0 or ns <= 0 or first <= 0:
            raise ValueError("ns, chunk and first must be > 0")
        k = 0
        while k < ns:
            n = min(first if k == 0 else chunk, ns - k)
            lin, q, err, smp, cnt = self.render_adaptive(nx, ny, k, n, eps, depth, seed, precision, region)
            k += n
            active = self.ctx.adaptive_status()[0]
            yield k, lin, q, err, smp, cnt, active
            if active == 0:
                break

    # ---- first-hit feature buffers and the denoised frame ------------------------------------------------------------------------------
    def render_features(self, nx, ny, na=FEATURE_SAMPLES, seed=RENDER_SEED, precision="f64", region=None):
        """-> (features float64 [h,w,8] = albedo rgb, normal xyz, depth, coverage: the mean over the first segments of render samples 0 .. na-1,
        counters {feature rays, pixels})"""
        x0, y0, x1, y1 = region if region is not None else (0, 0, nx, ny)
        ft = np.zeros((max(y1 - y0, 0), max(x1 - x0, 0), _ffi.FEATURES), np.float64)
        cnt = np.zeros(2, np.uint64)
        check(_ffi.lib().rtmi_render_features(self.handle, nx, ny, na, seed, _PRECISION[precision], x0, y0, x1, y1, ptr(ft), ptr(cnt)))
        return ft, cnt

    def render_features_device(self, nx, ny, na, out_features, out_counters=None, seed=RENDER_SEED, precision="f64", stream=None):
        """render_features for the whole frame into HBM-resident buffers (asynchronous, render_device's stream semantics)"""
        check(_ffi.lib().rtmi_render_features_device(self.handle, nx, ny, na, seed, _PRECISION[precision], ptr(out_features), ptr(out_counters),
                                                     ptr(stream)))

    def render_denoised(self, nx, ny, ns, na=FEATURE_SAMPLES, depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", **denoise):
        """One frame of ns samples with its noise estimate (render_progressive), its features (render_features, na samples) and the filtered frame
        (Context.denoise; keyword arguments: iterations, sigma_c, sigma_n, sigma_a, sigma_d) ->
        ((linear, rgb8, stderr, counters), features, (linear, rgb8, stderr) filtered).  The raw frame equals render(ns)."""
        try:
            raw = self.render_progressive(nx, ny, 0, ns, depth, seed, precision)
        finally:
            self.ctx.progressive_release()
        ft, _ = self.render_features(nx, ny, na, seed, precision)
        return raw, ft, self.ctx.denoise(raw[0], raw[2], ft, **denoise)

    def refine_adaptive_denoised(self, nx, ny, ns, chunk, eps, first=None, na=FEATURE_SAMPLES, iterations=DENOISE_ITERATIONS,
                                 sigma_c=DENOISE_SIGMA_C, sigma_n=DENOISE_SIGMA_N, sigma_a=DENOISE_SIGMA_A, sigma_d=DENOISE_SIGMA_D,
                                 depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64"):
        """Adaptive sampling steered by the noise estimate of the DENOISED frame: for a frame that will be filtered anyway, a tile stops taking
        samples once the filter has cleaned it.  The feature buffers are rendered once (na samples); then per round: render_adaptive with the raw
        rule at eps 0 (it retires only tiles whose samples are all equal), denoise of the frame with its standard error and the features,
        adaptive_retire of the tiles whose filtered standard error is <= eps everywhere.  Yields (k, linear, rgb8, stderr, samples, counters,
        active tiles after the retirement, filtered linear, filtered rgb8, filtered stderr) after every round and ends at ns or when no tile is
        active, like refine_adaptive.  Whole frame only (the filter is a whole-frame operation).  Every tile of the unfiltered frame equals
        render(ns = the samples it holds); the filtered frame is denoise of that frame."""
        first = chunk if first is None else first
        if chunk <= 0 or ns <= 0 or first <= 0:
            raise ValueError("ns, chunk and first must be > 0")
        ft, _ = self.render_features(nx, ny, na, seed, precision)
        k = 0
        while k < ns:
            n = min(first if k == 0 else chunk, ns - k)
            lin, q, err, smp, cnt = self.render_adaptive(nx, ny, k, n, 0.0, depth, seed, precision)
            k += n
            flt, fq, ferr = self.ctx.denoise(lin, err, ft, iterations, sigma_c, sigma_n, sigma_a, sigma_d)
            self.ctx.adaptive_retire(ferr, eps)
            active = self.ctx.adaptive_status()[0]
            yield k, lin, q, err, smp, cnt, active, flt, fq, ferr
            if active == 0:
                break

    def render_tiles_device(self, nx, ny, ns, tile_first, tile_stride, out_tiles, out_counters=None, depth=DEFAULT_DEPTH,
                            seed=RENDER_SEED, precision="f64", stream=None):
        check(_ffi.lib().rtmi_render_tiles_device(self.handle, nx, ny, ns, depth, seed, _PRECISION[precision],
                                                  tile_first, tile_stride, ptr(out_tiles), ptr(out_counters), ptr(stream)))

    def render_adaptive_tiles_device(self, nx, ny, s_first, s_count, retire, eps, tile_first, tile_stride, out_tiles_rec=None, out_counters=None,
                                     depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", stream=None):
        """The per-device primitive of a progressive / adaptive frame on several GPUs: samples [s_first, s_first + s_count) into the context's
        frame over the dealt tiles tile_first, tile_first + tile_stride, ... (retire: render_adaptive's two steps with eps, else
        render_progressive's one), the tiles' records [local tiles, 64, 5] float64 (mean rgb, stderr, samples) into out_tiles_rec and
        {segments so far, pixels of the dealt tiles} into out_counters, both HBM-resident.  Synchronises the stream once, at its end."""
        check(_ffi.lib().rtmi_render_adaptive_tiles_device(self.handle, nx, ny, s_first, s_count, int(retire), float(eps), depth, seed,
                                                           _PRECISION[precision], tile_first, tile_stride, ptr(out_tiles_rec), ptr(out_counters),
                                                           ptr(stream)))

    # ---- caller-supplied rays: panoramas, orthographic views, bakers, probes ------------------------------------------------------------
    @staticmethod
    def _rays_inputs(rays, group, keys, state):
        """render_rays' and render_rays_nee's arrays -> (rays [n, 7], group, n_groups, keys [n] or None); a state must have its layout"""
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 7)
        group = int(group)
        if group <= 0 or len(rays) % group:
            raise ValueError("%d rays are not whole groups of %d" % (len(rays), group))
        n_groups = len(rays) // group
        if keys is not None:
            keys = np.ascontiguousarray(keys, np.uint64).reshape(-1)
            if len(keys) != len(rays):
                raise ValueError("%d keys for %d rays" % (len(keys), len(rays)))
        if state is not None and (not isinstance(state, np.ndarray) or state.dtype != np.float64 or not state.flags.c_contiguous
                                  or state.shape != (n_groups, _ffi.RAYS_REC)):
            raise ValueError("state must be a C-contiguous float64 array [n_groups, %d]" % _ffi.RAYS_REC)
        return rays, group, n_groups, keys

    def _fold_chunks(self, nx, ny, ns, chunk, rays_of, trace, n_counters, **trace_args):
        """An nx x ny x ns image in chunks of `chunk` samples per pixel folded into one state: rays_of(k, n) -> (rays, ctr0) for samples
        [k, k + n) of every pixel, grouped per pixel; trace = render_rays or render_rays_nee -> (linear, rgb8, stderr, the counters summed)"""
        state = np.zeros((nx * ny, _ffi.RAYS_REC), np.float64)
        total = np.zeros(n_counters, np.uint64)
        k = 0
        while k < ns:
            n = min(chunk, ns - k)
            rays, ctr0 = rays_of(k, n)
            mean, err, cnt, _ = trace(rays, group=n, ctr0=ctr0, first=k, state=state, **trace_args)
            total += cnt
            k += n
        lin = np.ascontiguousarray(mean.reshape(ny, nx, 3)[::-1])  # group j * nx + i, j = 0 at the bottom
        return lin, self.ctx.denoise(lin, iterations=0)[1], np.ascontiguousarray(err.reshape(ny, nx)[::-1]), total

    def render_rays(self, rays, group=1, keys=None, seed=RENDER_SEED, ctr0=0, depth=DEFAULT_DEPTH, precision="f64", first=0, state=None,
                    return_rays=False):
        """One path per ray: rays [n_groups * group, 7] = origin, direction, time; ray r of group g is row g * group + r.  Its stream is keyed
        keys[row], or sample_key(seed, g, first + r) without keys, and starts at draw ctr0.  -> (mean [n_groups, 3] = the group's rays folded in
        row order as a frame folds a pixel's samples, stderr [n_groups] = render_progressive's noise estimate per group, counters {segments traced,
        rays}, rays' radiance [n, 3] or None).  state ([n_groups, RAYS_REC] float64, updated in place; first = 0 starts it, first > 0 continues
        it and must be the rays every group already holds): mean and stderr are then over all rays so far, and any split of a group's rays into
        consecutive calls gives the bits of one call."""
        rays, group, n_groups, keys = self._rays_inputs(rays, group, keys, state)
        mean, err, cnt = np.zeros((n_groups, 3), np.float64), np.zeros(n_groups, np.float64), np.zeros(2, np.uint64)
        out = np.zeros((len(rays), 3), np.float64) if return_rays else None
        check(_ffi.lib().rtmi_render_rays(self.handle, _PRECISION[precision], n_groups, group, int(first), ptr(rays), ptr(keys), int(seed), int(ctr0),
                                          int(depth), ptr(state), ptr(mean), ptr(err), ptr(out), ptr(cnt)))
        return mean, err, cnt, out

    def render_rays_device(self, n_groups, group, rays, out_mean, out_stderr, keys=None, seed=RENDER_SEED, ctr0=0, depth=DEFAULT_DEPTH,
                           precision="f64", first=0, state=None, out_rays=None, out_counters=None, stream=None):
        """render_rays on HBM-resident buffers (torch tensors or raw device pointers; asynchronous, render_device's stream semantics).  A state's
        count is the caller's contract: it is not read back."""
        check(_ffi.lib().rtmi_render_rays_device(self.handle, _PRECISION[precision], int(n_groups), int(group), int(first), ptr(rays), ptr(keys), int(seed),
                                                 int(ctr0), int(depth), ptr(state), ptr(out_mean), ptr(out_stderr), ptr(out_rays), ptr(out_counters),
                                                 ptr(stream)))

    def render_with(self, generator, nx, ny, ns, chunk, depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", nee=False, lights=None, light_choice=0,
                    **generator_args):
        """An nx x ny x ns image through a ray generator of camera.py (generator(nx, ny, s_first, s_count, seed=, **generator_args) -> (rays,
        ctr0), grouped per pixel): chunks of `chunk` samples per pixel folded into one state, keys derived from (seed, pixel, sample) ->
        (linear [ny, nx, 3] = the per-pixel mean, rgb8 = the frame's 8-bit quantiser of it (Context.denoise with no pass), stderr [ny, nx], counters
        summed over the chunks); row 0 = top.  The result does not depend on `chunk`.  nee: the paths sample the lights (render_rays_nee with
        `lights`; four counters); nee="mis": under multiple importance sampling (render_rays_mis with `lights` and `light_choice`); nee="ris":
        under the proposal rule (render_rays_ris with `lights`)."""
        if chunk <= 0 or ns <= 0:
            raise ValueError("ns and chunk must be > 0")
        def rays_of(k, n):
            return generator(nx, ny, k, n, seed=seed, **generator_args)
        if isinstance(nee, str) and nee in ("vol-nee", "vol-mis"):  # the volume rule: scenes that hold a ConstantMedium
            return self._fold_chunks(nx, ny, ns, chunk, rays_of, self.render_rays_vol, 4, estimator=nee[4:], lights=lights, light_choice=light_choice,
                                     seed=seed, depth=depth, precision=precision)
        if isinstance(nee, str) and nee == "ris":  # the proposal rule: every light proposes a point (light_choice is not looked at)
            return self._fold_chunks(nx, ny, ns, chunk, rays_of, self.render_rays_ris, 4, lights=lights, seed=seed, depth=depth, precision=precision)
        if isinstance(nee, str):
            if nee != "mis":
                raise ValueError("nee is False, True, \"mis\", \"ris\", \"vol-nee\" or \"vol-mis\" (got %r)" % nee)
            return self._fold_chunks(nx, ny, ns, chunk, rays_of, self.render_rays_mis, 4, lights=lights, light_choice=light_choice, seed=seed, depth=depth,
                                     precision=precision)
        if nee:
            return self._fold_chunks(nx, ny, ns, chunk, rays_of, self.render_rays_nee, 4, lights=lights, seed=seed, depth=depth, precision=precision)
        return self._fold_chunks(nx, ny, ns, chunk, rays_of, self.render_rays, 2, seed=seed, depth=depth, precision=precision)

    # ---- path tracing with next-event estimation: render_rays whose Lambertian vertices also sample the area lights -------------------------
    def render_rays_nee(self, rays, group=1, lights=None, keys=None, seed=RENDER_SEED, ctr0=0, depth=DEFAULT_DEPTH, precision="f64", first=0,
                        state=None, return_rays=False):
        """render_rays with one shadow ray per Lambertian vertex towards a sampled point of one uniformly chosen light (lights: primitive
        indices out of self.lights(); None: all of them) -- the NEE rule of include/rtmi.h, which camera.nee_samples restates.  The path itself
        (stream, hits, scatters, segments) is render_rays' bit for bit and the estimate has the same expectation; on a lit scene its variance is
        a fraction.  No lights: the call is render_rays.  A scene with a ConstantMedium is refused.  -> render_rays' tuple, the counters being
        {segments, rays, shadow rays built, shadow rays occluded}."""
        rays, group, n_groups, keys = self._rays_inputs(rays, group, keys, state)
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        mean, err, cnt = np.zeros((n_groups, 3), np.float64), np.zeros(n_groups, np.float64), np.zeros(4, np.uint64)
        out = np.zeros((len(rays), 3), np.float64) if return_rays else None
        check(_ffi.lib().rtmi_render_rays_nee(self.handle, _PRECISION[precision], n_groups, group, int(first), ptr(rays), ptr(keys), int(seed), int(ctr0),
                                              int(depth), n_listed, ptr(lights), ptr(state), ptr(mean), ptr(err), ptr(out), ptr(cnt)))
        return mean, err, cnt, out

    def render_rays_nee_device(self, n_groups, group, rays, out_mean, out_stderr, lights=None, keys=None, seed=RENDER_SEED, ctr0=0,
                               depth=DEFAULT_DEPTH, precision="f64", first=0, state=None, out_rays=None, out_counters=None, stream=None):
        """render_rays_nee on HBM-resident buffers (lights stays a host list; out_counters: four uint64); asynchronous, render_device's stream
        semantics.  A state's count is the caller's contract: it is not read back."""
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        check(_ffi.lib().rtmi_render_rays_nee_device(self.handle, _PRECISION[precision], int(n_groups), int(group), int(first), ptr(rays), ptr(keys),
                                                     int(seed), int(ctr0), int(depth), n_listed, ptr(lights), ptr(state), ptr(out_mean), ptr(out_stderr),
                                                     ptr(out_rays), ptr(out_counters), ptr(stream)))

    # ---- multiple importance sampling: the light sample and the scatter share each lamp's emission (THE MIS RULE of include/rtmi.h) ----------
    @staticmethod
    def _light_choice(light_choice):
        """0 / "uniform", 1 / "power" -> the C entry's light_choice (anything else goes through as an integer and is refused there)"""
        return MIS_CHOICES[light_choice] if isinstance(light_choice, str) else int(light_choice)

    def render_rays_mis(self, rays, group=1, lights=None, light_choice=0, keys=None, seed=RENDER_SEED, ctr0=0, depth=DEFAULT_DEPTH, precision="f64",
                        first=0, state=None, return_rays=False):
        """render_rays_nee under multiple importance sampling (rtmi_render_rays_mis): the same path and the same shadow rays, but the light sample
        counts with the balance heuristic's share m = x / (1 + x), x = p_scatter / p_light, and a closing emission on a sampled light -- which
        render_rays_nee drops -- with the scatter's share, so every contribution is at most T * Le: no bright outliers beside a lamp.
        light_choice: 0 / "uniform" or 1 / "power" (the light is picked in proportion to area x (Le.r + Le.g + Le.b)).  camera.mis_pick,
        mis_weight, mis_lobe and mis_closing restate the rule.  -> render_rays_nee's tuple."""
        rays, group, n_groups, keys = self._rays_inputs(rays, group, keys, state)
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        mean, err, cnt = np.zeros((n_groups, 3), np.float64), np.zeros(n_groups, np.float64), np.zeros(4, np.uint64)
        out = np.zeros((len(rays), 3), np.float64) if return_rays else None
        check(_ffi.lib().rtmi_render_rays_mis(self.handle, _PRECISION[precision], n_groups, group, int(first), ptr(rays), ptr(keys), int(seed), int(ctr0),
                                              int(depth), n_listed, ptr(lights), self._light_choice(light_choice), ptr(state), ptr(mean), ptr(err),
                                              ptr(out), ptr(cnt)))
        return mean, err, cnt, out

    def render_rays_mis_device(self, n_groups, group, rays, out_mean, out_stderr, lights=None, light_choice=0, keys=None, seed=RENDER_SEED, ctr0=0,
                               depth=DEFAULT_DEPTH, precision="f64", first=0, state=None, out_rays=None, out_counters=None, stream=None):
        """render_rays_mis on HBM-resident buffers (lights stays a host list; out_counters: four uint64); asynchronous, render_device's stream
        semantics.  A state's count is the caller's contract: it is not read back."""
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        check(_ffi.lib().rtmi_render_rays_mis_device(self.handle, _PRECISION[precision], int(n_groups), int(group), int(first), ptr(rays), ptr(keys),
                                                     int(seed), int(ctr0), int(depth), n_listed, ptr(lights), self._light_choice(light_choice), ptr(state),
                                                     ptr(out_mean), ptr(out_stderr), ptr(out_rays), ptr(out_counters), ptr(stream)))

    # ---- every lamp proposes a point, one shadow ray is sent: importance choice among the lights (THE PROPOSAL RULE of include/rtmi.h) ----------
    def render_rays_ris(self, rays, group=1, lights=None, keys=None, seed=RENDER_SEED, ctr0=0, depth=DEFAULT_DEPTH, precision="f64", first=0,
                        state=None, return_rays=False):
        """render_rays_mis whose light is chosen by looking at the vertex (rtmi_render_rays_ris): every listed light (at most DIRECT_MAX_LIGHTS)
        proposes one point, each proposal is weighed by lum * m -- what it would contribute if it were visible -- and a one-pass weighted reservoir
        keeps one, whose shadow ray counts with S / w^ on top of the balance heuristic's share.  The path and the closing emission are
        render_rays_mis'; with one lamp so is every bit of the result.  camera.ris_candidates and ris_choose restate the rule.
        -> render_rays_nee's tuple."""
        rays, group, n_groups, keys = self._rays_inputs(rays, group, keys, state)
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        mean, err, cnt = np.zeros((n_groups, 3), np.float64), np.zeros(n_groups, np.float64), np.zeros(4, np.uint64)
        out = np.zeros((len(rays), 3), np.float64) if return_rays else None
        check(_ffi.lib().rtmi_render_rays_ris(self.handle, _PRECISION[precision], n_groups, group, int(first), ptr(rays), ptr(keys), int(seed), int(ctr0),
                                              int(depth), n_listed, ptr(lights), ptr(state), ptr(mean), ptr(err), ptr(out), ptr(cnt)))
        return mean, err, cnt, out

    def render_rays_ris_device(self, n_groups, group, rays, out_mean, out_stderr, lights=None, keys=None, seed=RENDER_SEED, ctr0=0,
                               depth=DEFAULT_DEPTH, precision="f64", first=0, state=None, out_rays=None, out_counters=None, stream=None):
        """render_rays_ris on HBM-resident buffers (lights stays a host list; out_counters: four uint64); asynchronous, render_device's stream
        semantics.  A state's count is the caller's contract: it is not read back."""
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        check(_ffi.lib().rtmi_render_rays_ris_device(self.handle, _PRECISION[precision], int(n_groups), int(group), int(first), ptr(rays), ptr(keys),
                                                     int(seed), int(ctr0), int(depth), n_listed, ptr(lights), ptr(state), ptr(out_mean), ptr(out_stderr),
                                                     ptr(out_rays), ptr(out_counters), ptr(stream)))

    def render_lit_ris(self, nx, ny, ns, chunk=None, lights=None, depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", return_rays=False,
                       return_camera=False, tiles=None, s_first=0, linear=None, rgb8=None, stderr=None, state=None):
        """The frame of the scene's own camera under the proposal rule (rtmi_render_lit_ris).  tiles None: render_lit's call and tuple -- an
        nx x ny x ns frame, `chunk` samples per call through one state.  tiles (int32, strictly ascending global tile indices): render_lit_tiles'
        call -- samples [s_first, s_first + ns) of the listed tiles' pixels folded IN PLACE into the caller's whole-frame linear, rgb8 (or None),
        stderr and state (or None) -> render_lit_tiles' tuple (counters[, rays][, camera]) in THE TILE ORDER."""
        nx, ny, ns = int(nx), int(ny), int(ns)
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        entry = _ffi.lib().rtmi_render_lit_ris
        if tiles is not None:
            tiles = np.ascontiguousarray(tiles, np.int32).reshape(-1)
            for name, a, shape, dt in (("linear", linear, (ny, nx, 3), np.float64), ("rgb8", rgb8, (ny, nx, 3), np.uint8),
                                       ("stderr", stderr, (ny, nx), np.float64), ("state", state, (nx * ny, _ffi.RAYS_REC), np.float64)):
                if (a is None and name in ("linear", "stderr")) or (
                        a is not None and not (isinstance(a, np.ndarray) and a.dtype == dt and a.shape == shape and a.flags.c_contiguous)):
                    raise ValueError("%s must be a contiguous %s array of shape %r: it is written in place" % (name, np.dtype(dt).name, shape))
            cnt = np.zeros(4, np.uint64)
            rays = np.zeros((len(tiles) * 64, ns, 3), np.float64) if return_rays else None
            cam = np.zeros((len(tiles) * 64, ns, 8), np.float64) if return_camera else None
            held = tiles if len(tiles) else np.zeros(1, np.int32)  # (an empty list is still a list: a pointer that is not NULL)
            check(entry(self.handle, _PRECISION[precision], nx, ny, int(s_first), ns, int(depth), int(seed), n_listed, ptr(lights), len(tiles), ptr(held),
                        ptr(state), ptr(linear), ptr(rgb8), ptr(stderr), ptr(rays), ptr(cam), ptr(cnt)))
            return (cnt,) + ((rays,) if return_rays else ()) + ((cam,) if return_camera else ())
        chunk = ns if chunk is None else int(chunk)
        if nx <= 0 or ny <= 0 or ns <= 0 or chunk <= 0:
            raise ValueError("nx, ny, ns and chunk must be > 0")
        npx = nx * ny
        lin, q, err = np.zeros((ny, nx, 3), np.float64), np.zeros((ny, nx, 3), np.uint8), np.zeros((ny, nx), np.float64)
        state = np.zeros((npx, _ffi.RAYS_REC), np.float64) if chunk < ns else None
        total = np.zeros(4, np.uint64)
        rays = np.zeros((npx, ns, 3), np.float64) if return_rays else None
        cam = np.zeros((npx, ns, 8), np.float64) if return_camera else None
        k = 0
        while k < ns:
            n = min(chunk, ns - k)
            cnt = np.zeros(4, np.uint64)
            r = np.zeros((npx, n, 3), np.float64) if return_rays else None
            c = np.zeros((npx, n, 8), np.float64) if return_camera else None
            check(entry(self.handle, _PRECISION[precision], nx, ny, k, n, int(depth), int(seed), n_listed, ptr(lights), 0, None,
                        ptr(state), ptr(lin), ptr(q), ptr(err), ptr(r), ptr(c), ptr(cnt)))
            total += cnt
            if return_rays:
                rays[:, k:k + n] = r
            if return_camera:
                cam[:, k:k + n] = c
            k += n
        return (lin, q, err, total) + ((rays,) if return_rays else ()) + ((cam,) if return_camera else ())

    def render_lit_ris_device(self, nx, ny, s_first, s_count, out_linear, out_stderr, out_rgb8=None, lights=None, n_tiles=0, tiles=None,
                              depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", state=None, out_rays=None, out_camera=None, out_counters=None,
                              stream=None):
        """rtmi_render_lit_ris_device on HBM-resident buffers: tiles None is render_lit_device's call, a device int32 list (its first n_tiles
        entries) render_lit_tiles_device's; asynchronous, render_device's stream semantics."""
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        check(_ffi.lib().rtmi_render_lit_ris_device(self.handle, _PRECISION[precision], int(nx), int(ny), int(s_first), int(s_count), int(depth), int(seed),
                                                    n_listed, ptr(lights), int(n_tiles), ptr(tiles), ptr(state), ptr(out_linear), ptr(out_rgb8),
                                                    ptr(out_stderr), ptr(out_rays), ptr(out_camera), ptr(out_counters), ptr(stream)))

    # ---- light-sampled paths through participating media (THE VOLUME RULE of include/rtmi.h) -------------------------------------------------
    @staticmethod
    def _vol_estimator(estimator):
        """"nee" / "mis" (or 1 / 2) -> the C entry's estimator; an unknown name is a ValueError, before any device work (an integer goes through
        and is refused there)"""
        if isinstance(estimator, str):
            if estimator not in VOL_ESTIMATORS:
                raise ValueError("estimator is one of %s (got %r)" % (", ".join(sorted(VOL_ESTIMATORS)), estimator))
            return VOL_ESTIMATORS[estimator]
        return int(estimator)

    def render_rays_vol(self, rays, group=1, estimator="mis", lights=None, light_choice=0, keys=None, seed=RENDER_SEED, ctr0=0, depth=DEFAULT_DEPTH,
                        precision="f64", first=0, state=None, return_rays=False):
        """render_rays_nee (estimator "nee" / 1) or render_rays_mis ("mis" / 2) on a scene that holds a ConstantMedium (rtmi_render_rays_vol): the
        Isotropic scatters inside a medium sample the lights too, with the uniform sphere's density 1 / 4 pi in the lobe's place, and every shadow
        ray draws from a stream of its own (sample_key(K, j, 2)) the free-flight distances of the media it crosses, so its unoccluded flag is an
        unbiased estimate of the transmittance.  camera.vol_samples and vol_lobe restate the rule.  Without media the result is the sibling's bit
        for bit.  -> render_rays_nee's tuple."""
        est = self._vol_estimator(estimator)
        rays, group, n_groups, keys = self._rays_inputs(rays, group, keys, state)
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        mean, err, cnt = np.zeros((n_groups, 3), np.float64), np.zeros(n_groups, np.float64), np.zeros(4, np.uint64)
        out = np.zeros((len(rays), 3), np.float64) if return_rays else None
        check(_ffi.lib().rtmi_render_rays_vol(self.handle, _PRECISION[precision], n_groups, group, int(first), ptr(rays), ptr(keys), int(seed), int(ctr0),
                                              int(depth), est, n_listed, ptr(lights), self._light_choice(light_choice),
                                              ptr(state), ptr(mean), ptr(err), ptr(out), ptr(cnt)))
        return mean, err, cnt, out

    def render_rays_vol_device(self, n_groups, group, rays, out_mean, out_stderr, estimator="mis", lights=None, light_choice=0, keys=None,
                               seed=RENDER_SEED, ctr0=0, depth=DEFAULT_DEPTH, precision="f64", first=0, state=None, out_rays=None, out_counters=None,
                               stream=None):
        """render_rays_vol on HBM-resident buffers (lights stays a host list; out_counters: four uint64); asynchronous, render_device's stream
        semantics.  A state's count is the caller's contract: it is not read back."""
        est = self._vol_estimator(estimator)
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        check(_ffi.lib().rtmi_render_rays_vol_device(self.handle, _PRECISION[precision], int(n_groups), int(group), int(first), ptr(rays), ptr(keys),
                                                     int(seed), int(ctr0), int(depth), est, n_listed, ptr(lights),
                                                     self._light_choice(light_choice), ptr(state), ptr(out_mean), ptr(out_stderr), ptr(out_rays),
                                                     ptr(out_counters), ptr(stream)))

    def render_lit_vol(self, nx, ny, ns, chunk=None, estimator="mis", lights=None, light_choice=0, depth=DEFAULT_DEPTH, seed=RENDER_SEED,
                       precision="f64", return_rays=False, return_camera=False):
        """render_lit under the volume rule (rtmi_render_lit_vol; estimator "nee" or "mis" only): the frame of a scene that holds a ConstantMedium
        -- make-final, the smoke Cornell box, make-subsurface-sphere -- through light-sampled paths.  -> render_lit's tuple."""
        return self.render_lit(nx, ny, ns, chunk, self._vol_estimator(estimator), lights, light_choice, depth, seed, precision, return_rays,
                               return_camera, _entry=_ffi.lib().rtmi_render_lit_vol)

    def render_lit_vol_device(self, nx, ny, s_first, s_count, out_linear, out_stderr, out_rgb8=None, estimator="mis", lights=None, light_choice=0,
                              depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", state=None, out_rays=None, out_camera=None, out_counters=None,
                              stream=None):
        """rtmi_render_lit_vol_device: render_lit_device under the volume rule (estimator "nee" or "mis" only)."""
        est = self._vol_estimator(estimator)
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        check(_ffi.lib().rtmi_render_lit_vol_device(self.handle, _PRECISION[precision], int(nx), int(ny), int(s_first), int(s_count), int(depth), int(seed),
                                                    est, n_listed, ptr(lights), self._light_choice(light_choice), ptr(state),
                                                    ptr(out_linear), ptr(out_rgb8), ptr(out_stderr), ptr(out_rays), ptr(out_camera), ptr(out_counters),
                                                    ptr(stream)))

    def render_nee(self, nx, ny, ns, chunk, depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", lights=None, mis=False, light_choice=0):
        """An nx x ny x ns frame of the scene's own camera (of either kind) through light-sampled paths, folded per pixel through one state as
        render_with folds.  Film jitter, lens draws and path streams come from three seeds derived from `seed` (sample_key(seed, 0 / 1 / 2, 0)),
        so none of them shares draws with another: sample s of pixel g jitters with draws 0 and 1 of sample_key(film, g, s), its camera ray is
        probe_camera's for that (u, v) with the stream sample_key(lens, g, s), and its path is keyed sample_key(paths, g, s) from draw 0.
        -> render_with's tuple (four counters); the result does not depend on `chunk`.  mis: the same rays and paths through render_rays_mis with
        `light_choice`."""
        from . import util
        if nx <= 0 or ny <= 0 or chunk <= 0 or ns <= 0:
            raise ValueError("nx, ny, ns and chunk must be > 0")
        film, lens, paths = (util.sample_key(seed, k, 0) for k in range(3))

        def rays_of(k, n):
            pix, ss = (a.ravel() for a in np.meshgrid(np.arange(nx * ny), np.arange(k, k + n), indexing="ij"))
            fk = util.sample_keys(film, pix, ss)
            u = ((pix % nx).astype(np.float64) + util.draw_uniforms(fk, 0)) / np.float64(nx)
            v = ((pix // nx).astype(np.float64) + util.draw_uniforms(fk, 1)) / np.float64(ny)
            return self.probe_camera(np.stack([u, v], axis=1), util.sample_keys(lens, pix, ss), precision=precision)[:, :7], 0
        if mis:
            return self._fold_chunks(nx, ny, ns, chunk, rays_of, self.render_rays_mis, 4, lights=lights, light_choice=light_choice, seed=paths, depth=depth,
                                     precision=precision)
        return self._fold_chunks(nx, ny, ns, chunk, rays_of, self.render_rays_nee, 4, lights=lights, seed=paths, depth=depth, precision=precision)

    # ---- light-sampled frames of the scene's own camera, the rays built on the device (THE FRAME RULE of include/rtmi.h) ----------------------
    @staticmethod
    def _lit_estimator(estimator):
        """"plain" / "nee" / "mis" (or 0 / 1 / 2) -> the C entry's estimator; an unknown name is a ValueError, before any device work"""
        if isinstance(estimator, str):
            if estimator not in LIT_ESTIMATORS:
                raise ValueError("estimator is one of %s (got %r)" % (", ".join(sorted(LIT_ESTIMATORS)), estimator))
            return LIT_ESTIMATORS[estimator]
        if isinstance(estimator, bool) or int(estimator) not in (0, 1, 2):
            raise ValueError("estimator is 0 (plain), 1 (nee) or 2 (mis) (got %r)" % (estimator,))
        return int(estimator)

    def render_lit(self, nx, ny, ns, chunk=None, estimator="mis", lights=None, light_choice=0, depth=DEFAULT_DEPTH, seed=RENDER_SEED,
                   precision="f64", return_rays=False, return_camera=False, _entry=None):
        """An nx x ny x ns frame of the scene's own camera through rtmi_render_lit: the paths `render` traces -- the same keys, film jitter, lens
        draws and streams, built on the device, no ray uploaded -- under the plain estimator ("plain": the frame of `render` bit for bit), the NEE
        rule ("nee") or the MIS rule ("mis", with light_choice 0 / "uniform" or 1 / "power").  chunk: samples per call, folded through one state
        (None: one call); the result does not depend on it.  -> (linear [ny, nx, 3], rgb8, stderr [ny, nx], counters {segments, rays, shadow rays
        built, shadow rays occluded} summed over the calls[, rays' radiance [nx * ny, ns, 3]][, camera [nx * ny, ns, 8] = origin, direction,
        time, the stream position behind the camera]); row 0 = top."""
        est = self._lit_estimator(estimator) if _entry is None else int(estimator)  # (_entry: render_lit_vol's C entry, the same arguments)
        entry = _ffi.lib().rtmi_render_lit if _entry is None else _entry
        nx, ny, ns = int(nx), int(ny), int(ns)
        chunk = ns if chunk is None else int(chunk)
        if nx <= 0 or ny <= 0 or ns <= 0 or chunk <= 0:
            raise ValueError("nx, ny, ns and chunk must be > 0")
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        choice = self._light_choice(light_choice)
        npx = nx * ny
        lin, q, err = np.zeros((ny, nx, 3), np.float64), np.zeros((ny, nx, 3), np.uint8), np.zeros((ny, nx), np.float64)
        state = np.zeros((npx, _ffi.RAYS_REC), np.float64) if chunk < ns else None
        total = np.zeros(4, np.uint64)
        rays = np.zeros((npx, ns, 3), np.float64) if return_rays else None
        cam = np.zeros((npx, ns, 8), np.float64) if return_camera else None
        k = 0
        while k < ns:
            n = min(chunk, ns - k)
            cnt = np.zeros(4, np.uint64)
            r = np.zeros((npx, n, 3), np.float64) if return_rays else None
            c = np.zeros((npx, n, 8), np.float64) if return_camera else None
            check(entry(self.handle, _PRECISION[precision], nx, ny, k, n, int(depth), int(seed), est, n_listed, ptr(lights), choice,
                        ptr(state), ptr(lin), ptr(q), ptr(err), ptr(r), ptr(c), ptr(cnt)))
            total += cnt
            if return_rays:
                rays[:, k:k + n] = r
            if return_camera:
                cam[:, k:k + n] = c
            k += n
        return (lin, q, err, total) + ((rays,) if return_rays else ()) + ((cam,) if return_camera else ())

    def render_lit_device(self, nx, ny, s_first, s_count, out_linear, out_stderr, out_rgb8=None, estimator="mis", lights=None, light_choice=0,
                          depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", state=None, out_rays=None, out_camera=None, out_counters=None,
                          stream=None):
        """rtmi_render_lit_device: samples [s_first, s_first + s_count) of every pixel on HBM-resident buffers (torch tensors or raw device pointers;
        lights stays a host list; out_counters: four uint64); asynchronous, render_device's stream semantics.  state ([nx * ny, RAYS_REC] doubles,
        the caller's): the frame refined over calls; its count is the caller's contract and is not read back."""
        est = self._lit_estimator(estimator)
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        check(_ffi.lib().rtmi_render_lit_device(self.handle, _PRECISION[precision], int(nx), int(ny), int(s_first), int(s_count), int(depth), int(seed), est,
                                                n_listed, ptr(lights), self._light_choice(light_choice), ptr(state), ptr(out_linear), ptr(out_rgb8),
                                                ptr(out_stderr), ptr(out_rays), ptr(out_camera), ptr(out_counters), ptr(stream)))

    # ---- light-sampled frames over a caller's list of 8x8 tiles, and the adaptive loop on top (THE TILE ORDER of include/rtmi.h) --------------
    def _tiles_estimator(self, estimator, volume):
        return self._vol_estimator(estimator) if volume else self._lit_estimator(estimator)

    def render_lit_tiles(self, nx, ny, s_first, s_count, tiles, linear, rgb8, stderr, state=None, estimator="mis", volume=False, lights=None,
                         light_choice=0, depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", return_rays=False, return_camera=False):
        """rtmi_render_lit_tiles: samples [s_first, s_first + s_count) of the pixels of the listed tiles (int32, strictly ascending global tile
        indices) folded IN PLACE into the caller's whole-frame arrays linear [ny, nx, 3] float64, rgb8 [ny, nx, 3] uint8 (or None), stderr
        [ny, nx] float64 and state [nx * ny, RAYS_REC] (or None); no other element changes.  volume: the volume rule (render_lit_vol's).
        -> (counters[, rays' radiance [len(tiles) * 64, s_count, 3]][, camera [len(tiles) * 64, s_count, 8]]) in THE TILE ORDER, the rows of
        pixels outside the image zeros."""
        tiles = np.ascontiguousarray(tiles, np.int32).reshape(-1)
        for name, a, shape, dt in (("linear", linear, (ny, nx, 3), np.float64), ("rgb8", rgb8, (ny, nx, 3), np.uint8),
                                   ("stderr", stderr, (ny, nx), np.float64), ("state", state, (nx * ny, _ffi.RAYS_REC), np.float64)):
            if a is not None and not (isinstance(a, np.ndarray) and a.dtype == dt and a.shape == shape and a.flags.c_contiguous):
                raise ValueError("%s must be a contiguous %s array of shape %r: it is written in place" % (name, np.dtype(dt).name, shape))
        est = self._tiles_estimator(estimator, volume)
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        cnt = np.zeros(4, np.uint64)
        rays = np.zeros((len(tiles) * 64, int(s_count), 3), np.float64) if return_rays else None
        cam = np.zeros((len(tiles) * 64, int(s_count), 8), np.float64) if return_camera else None
        check(_ffi.lib().rtmi_render_lit_tiles(self.handle, _PRECISION[precision], int(nx), int(ny), int(s_first), int(s_count), int(depth), int(seed), est,
                                               n_listed, ptr(lights), self._light_choice(light_choice), int(bool(volume)), len(tiles), ptr(tiles),
                                               ptr(state), ptr(linear), ptr(rgb8), ptr(stderr), ptr(rays), ptr(cam), ptr(cnt)))
        return (cnt,) + ((rays,) if return_rays else ()) + ((cam,) if return_camera else ())

    def render_lit_tiles_device(self, nx, ny, s_first, s_count, n_tiles, tiles, out_linear, out_stderr, out_rgb8=None, estimator="mis", volume=False,
                                lights=None, light_choice=0, depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", state=None, out_rays=None,
                                out_camera=None, out_counters=None, stream=None):
        """rtmi_render_lit_tiles_device: render_lit_device over the first n_tiles entries of an HBM-resident int32 tile list; the frame buffers
        and the state are the whole frame's and only the listed pixels' elements are written.  An entry outside the frame holds no pixel;
        duplicates and order are the caller's contract."""
        est = self._tiles_estimator(estimator, volume)
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        check(_ffi.lib().rtmi_render_lit_tiles_device(self.handle, _PRECISION[precision], int(nx), int(ny), int(s_first), int(s_count), int(depth),
                                                      int(seed), est, n_listed, ptr(lights), self._light_choice(light_choice), int(bool(volume)),
                                                      int(n_tiles), ptr(tiles), ptr(state), ptr(out_linear), ptr(out_rgb8), ptr(out_stderr),
                                                      ptr(out_rays), ptr(out_camera), ptr(out_counters), ptr(stream)))

    def refine_lit_adaptive(self, nx, ny, ns, chunk, eps, first=None, estimator="mis", volume=False, lights=None, light_choice=0, denoised=False,
                            na=FEATURE_SAMPLES, iterations=DENOISE_ITERATIONS, sigma_c=DENOISE_SIGMA_C, sigma_n=DENOISE_SIGMA_N,
                            sigma_a=DENOISE_SIGMA_A, sigma_d=DENOISE_SIGMA_D, depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64"):
        """A light-sampled frame refined adaptively: every 8x8 tile listed, then rounds of render_lit_tiles (`first` samples, default chunk, then
        `chunk`) each followed by tiles_retire of the tiles whose standard error is <= eps everywhere -- with denoised=True of those whose FILTERED
        standard error is (render_features once, denoise per round, as refine_adaptive_denoised) -- until no tile is listed or ns is reached.
        estimator "ris": the rounds go through render_lit_ris (the proposal rule; volume and light_choice do not apply).
        -> (linear, rgb8, stderr, samples [ny, nx] int32, counters summed over the rounds, rounds = [(k, tiles listed after the round's
        retirement, int32)]).  A pixel whose tile took n samples equals render_lit(ns = n) there bit for bit.  With torch the buffers and the list
        stay in HBM across the rounds and only the number of survivors comes back per round."""
        first = chunk if first is None else first
        if nx <= 0 or ny <= 0 or chunk <= 0 or ns <= 0 or first <= 0:
            raise ValueError("nx, ny, ns, chunk and first must be > 0")
        n_all = ((nx + _ffi.TILE - 1) // _ffi.TILE) * ((ny + _ffi.TILE - 1) // _ffi.TILE)
        kw = dict(estimator=estimator, volume=volume, lights=lights, light_choice=light_choice, depth=depth, seed=seed, precision=precision)
        ris = isinstance(estimator, str) and estimator == "ris"  # the proposal rule's frame call: no estimator, light_choice or volume
        if ris and volume:
            raise ValueError("estimator \"ris\" has no volume form")
        kr = dict(lights=lights, depth=depth, seed=seed, precision=precision)
        dn = (int(iterations), float(sigma_c), float(sigma_n), float(sigma_a), float(sigma_d))
        total, rounds, k, n_tiles = np.zeros(4, np.uint64), [], 0, n_all
        if _ffi.torch is None:  # host arrays: every round stages the frame
            lin, q, err = np.zeros((ny, nx, 3), np.float64), np.zeros((ny, nx, 3), np.uint8), np.zeros((ny, nx), np.float64)
            state, tiles = np.zeros((nx * ny, _ffi.RAYS_REC), np.float64), np.arange(n_all, dtype=np.int32)
            ft = self.render_features(nx, ny, na, seed, precision)[0] if denoised else None
            while k < ns and len(tiles):
                n = min(first if k == 0 else chunk, ns - k)
                if ris:
                    total += self.render_lit_ris(nx, ny, n, tiles=tiles, s_first=k, linear=lin, rgb8=q, stderr=err, state=state, **kr)[0]
                else:
                    total += self.render_lit_tiles(nx, ny, k, n, tiles, lin, q, err, state, **kw)[0]
                k += n
                tiles = self.ctx.tiles_retire(self.ctx.denoise(lin, err, ft, *dn)[2] if denoised else err, eps, tiles)
                rounds.append((k, tiles))
            return lin, q, err, state[:, 9].reshape(ny, nx).astype(np.int32), total, rounds
        torch = _ffi.torch
        dev = torch.device("cuda", self.ctx.device)
        f64 = dict(dtype=torch.float64, device=dev)
        side = torch.cuda.Stream(dev)  # torch's own operations and the library's calls in one order
        stream = side.cuda_stream
        with torch.cuda.stream(side):
            lin, q, err = torch.zeros((ny, nx, 3), **f64), torch.zeros((ny, nx, 3), dtype=torch.uint8, device=dev), torch.zeros((ny, nx), **f64)
            state, tiles = torch.zeros((nx * ny, _ffi.RAYS_REC), **f64), torch.arange(n_all, dtype=torch.int32, device=dev)
            cnt, sums = torch.zeros(4, dtype=torch.int64, device=dev), torch.zeros(4, dtype=torch.int64, device=dev)
            ft = ferr = None
            if denoised:
                ft, ferr = torch.zeros((ny, nx, _ffi.FEATURES), **f64), torch.zeros((ny, nx), **f64)
                self.render_features_device(nx, ny, na, ft, None, seed, precision, stream)
            kept = []
            while k < ns and n_tiles:
                n = min(first if k == 0 else chunk, ns - k)
                if ris:
                    self.render_lit_ris_device(nx, ny, k, n, lin, err, q, n_tiles=n_tiles, tiles=tiles, state=state, out_counters=cnt, stream=stream, **kr)
                else:
                    self.render_lit_tiles_device(nx, ny, k, n, n_tiles, tiles, lin, err, q, state=state, out_counters=cnt, stream=stream, **kw)
                k += n
                if denoised:
                    self.ctx.denoise_device(nx, ny, lin, err, ft, None, None, ferr, *dn, stream=stream)
                n_tiles = self.ctx.tiles_retire_device(nx, ny, ferr if denoised else err, eps, n_tiles, tiles, stream=stream)  # (synchronises)
                sums += cnt
                kept.append((k, tiles[:n_tiles].clone()))
            side.synchronize()
            rounds = [(kk, t.cpu().numpy()) for kk, t in kept]
            return (lin.cpu().numpy(), q.cpu().numpy(), err.cpu().numpy(), state[:, 9].reshape(ny, nx).cpu().numpy().astype(np.int32),
                    sums.cpu().numpy().astype(np.uint64), rounds)

    # ---- closest-hit and any-hit queries: picking, first hits, shadow / ambient-occlusion / line-of-sight rays --------------------------------
    @staticmethod
    def _query_inputs(rays, t_range, keys):
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 7)
        if t_range is not None:
            t_range = np.ascontiguousarray(t_range, np.float64).reshape(-1, 2)
            if len(t_range) != len(rays):
                raise ValueError("%d ranges for %d rays" % (len(t_range), len(rays)))
        if keys is not None:
            keys = np.ascontiguousarray(keys, np.uint64).reshape(-1)
            if len(keys) != len(rays):
                raise ValueError("%d keys for %d rays" % (len(keys), len(rays)))
        return rays, t_range, keys

    def query_hits(self, rays, t_min=T_MIN, t_max=T_MAX, t_range=None, keys=None, ctr0=0, precision="f64", return_counters=False):
        """The closest hit of every ray: rays [n, 7] = origin, direction, time -> [n, HIT_REC] float64 = hit?, prim, t, p xyz, normal xyz, u, v
        (probe_hit's record, bit for bit) and the hit primitive's material; zeros on a miss.  t_range [n, 2]: each ray's own (t-min, t-max) in place
        of the scalars.  keys (with ctr0): the streams a ConstantMedium draws from; None keys every ray 0, as probe_hit.  return_counters: also
        {rays, rays that hit}."""
        rays, t_range, keys = self._query_inputs(rays, t_range, keys)
        out, cnt = np.zeros((len(rays), _ffi.HIT_REC), np.float64), np.zeros(2, np.uint64)
        check(_ffi.lib().rtmi_query_hits(self.handle, _PRECISION[precision], len(rays), ptr(rays), ptr(t_range), float(t_min), float(t_max), ptr(keys),
                                         int(ctr0), ptr(out), ptr(cnt)))
        return (out, cnt) if return_counters else out

    def query_hits_device(self, n, rays, out_hits, t_min=T_MIN, t_max=T_MAX, t_range=None, keys=None, ctr0=0, precision="f64", out_counters=None,
                          stream=None):
        """query_hits on HBM-resident buffers (torch tensors or raw device pointers; asynchronous, render_device's stream semantics)"""
        check(_ffi.lib().rtmi_query_hits_device(self.handle, _PRECISION[precision], int(n), ptr(rays), ptr(t_range), float(t_min), float(t_max), ptr(keys),
                                                int(ctr0), ptr(out_hits), ptr(out_counters), ptr(stream)))

    def occluded(self, rays, group=1, t_min=T_MIN, t_max=T_MAX, t_range=None, keys=None, ctr0=0, precision="f64"):
        """Is anything hit within each ray's range?  rays [n_groups * group, 7], ray r of group g is row g * group + r -> (flags uint8 [n] = 1 where
        query_hits would report a hit, counts int32 [n_groups] = occluded rays per group, counters {rays, occluded rays}).  The search leaves at
        the first primitive that accepts the ray instead of looking for the nearest."""
        rays, t_range, keys = self._query_inputs(rays, t_range, keys)
        group = int(group)
        if group <= 0 or len(rays) % group:
            raise ValueError("%d rays are not whole groups of %d" % (len(rays), group))
        n_groups = len(rays) // group
        flags, counts, cnt = np.zeros(len(rays), np.uint8), np.zeros(n_groups, np.int32), np.zeros(2, np.uint64)
        check(_ffi.lib().rtmi_query_occluded(self.handle, _PRECISION[precision], n_groups, group, ptr(rays), ptr(t_range), float(t_min), float(t_max),
                                             ptr(keys), int(ctr0), ptr(flags), ptr(counts), ptr(cnt)))
        return flags, counts, cnt

    def occluded_device(self, n_groups, group, rays, out_occluded=None, out_count=None, t_min=T_MIN, t_max=T_MAX, t_range=None, keys=None, ctr0=0,
                        precision="f64", out_counters=None, stream=None):
        """occluded on HBM-resident buffers (uint8 flags, int32 counts; either may be None); asynchronous, render_device's stream semantics"""
        check(_ffi.lib().rtmi_query_occluded_device(self.handle, _PRECISION[precision], int(n_groups), int(group), ptr(rays), ptr(t_range), float(t_min),
                                                    float(t_max), ptr(keys), int(ctr0), ptr(out_occluded), ptr(out_count), ptr(out_counters),
                                                    ptr(stream)))

    def pixel_centre_rays(self, nx, ny, columns=None, rows=None):
        """The rays through pixel centres from the camera's origin (a thin lens: its lens centre, at shutter time t0): u = (i + 1/2) / nx, v =
        (ny - 1 - j + 1/2) / ny for column i and row j from the top, direction lleft + u horiz + v vert - origin in get-ray's operation order
        (step 1 of rtmi_reproject).  columns / rows: paired index arrays; default every pixel, row-major from the top -> rays [n, 7]."""
        info = self.camera_info()
        c = info["cam"]
        if columns is None:
            rows, columns = (a.ravel() for a in np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij"))
        i, j = np.asarray(columns, np.float64).ravel(), np.asarray(rows, np.float64).ravel()
        u, v = (i + 0.5) / np.float64(nx), ((np.float64(ny - 1) - j) + 0.5) / np.float64(ny)
        rays = np.empty((len(u), 7), np.float64)
        rays[:, 0:3] = c[0:3]
        rays[:, 3:6] = ((c[3:6] + c[6:9] * u[:, None]) + c[9:12] * v[:, None]) + (-c[0:3])
        rays[:, 6] = 0.0 if info["cam_kind"] == 0 else c[22]
        return rays

    def pick(self, nx, ny, i, j):
        """What lies under pixel (column i, row j from the top) of an nx x ny view: None, or {"prim", "material", "t", "p", "normal", "uv"} of the
        closest hit of the ray through the pixel's centre (pixel_centre_rays)."""
        if not (0 <= i < nx and 0 <= j < ny):
            raise ValueError("pixel (%d, %d) outside %d x %d" % (i, j, nx, ny))
        h = self.query_hits(self.pixel_centre_rays(nx, ny, [i], [j]))[0]
        if h[0] == 0.0:
            return None
        return {"prim": int(h[1]), "material": int(h[11]), "t": float(h[2]), "p": h[3:6].copy(), "normal": h[6:9].copy(), "uv": h[9:11].copy()}

    def ambient_occlusion(self, nx, ny, n_dirs, radius, seed=RENDER_SEED, chunk=None):
        """Ambient occlusion of the view: [ny, nx] float64 visibility, row 0 = top.  The first hits of the pixel-centre rays (query_hits_device), then
        n_dirs cosine-weighted rays per hit (camera.hemisphere_rays; point g = pixel j * nx + i, j from the top) from the hit point into the hemisphere
        on the viewer's side of the surface, t-range (0.001, radius), through occluded_device with one group per pixel: 1 - occluded / n_dirs, and
        1 where the primary ray missed.  chunk: directions per any-hit call (default all n_dirs); the result does not depend on it."""
        import torch

        from . import camera as cam
        if nx <= 0 or ny <= 0 or n_dirs <= 0:
            raise ValueError("nx, ny, n_dirs must be > 0")
        n = nx * ny
        dev = torch.device("cuda", self.ctx.device)
        primary = self.pixel_centre_rays(nx, ny)
        d_rays = torch.from_numpy(primary).to(dev)
        d_hits = torch.zeros((n, _ffi.HIT_REC), dtype=torch.float64, device=dev)
        torch.cuda.synchronize(dev)  # (uploads and fills ran on torch's stream; nothing of torch's is queued after this)
        self.query_hits_device(n, d_rays, d_hits)
        torch.cuda.synchronize(dev)  # (a device-wide wait: the context's stream included)
        hits = d_hits.cpu().numpy()
        hit = hits[:, 0] != 0.0
        normals = hits[:, 6:9].copy()
        away = (normals * primary[:, 3:6]).sum(axis=1) > 0.0  # the normal points away from the viewer: take the other side
        normals[away] = -normals[away]
        normals[~hit] = (0.0, 1.0, 0.0)  # (a missed pixel's rays are traced and ignored: every group keeps its place)
        chunk = n_dirs if chunk is None else max(1, int(chunk))
        occluded = np.zeros(n, np.int64)
        for first in range(0, n_dirs, chunk):
            m = min(chunk, n_dirs - first)
            rays = cam.hemisphere_rays(hits[:, 3:6], normals, m, first=first, seed=seed, time=primary[0, 6])
            d_sec = torch.from_numpy(rays).to(dev)
            d_count = torch.zeros(n, dtype=torch.int32, device=dev)
            torch.cuda.synchronize(dev)
            self.occluded_device(n, m, d_sec, out_count=d_count, t_min=T_MIN, t_max=float(radius))
            torch.cuda.synchronize(dev)
            occluded += d_count.cpu().numpy()
        vis = 1.0 - occluded.astype(np.float64) / float(n_dirs)
        vis[~hit] = 1.0
        return vis.reshape(ny, nx)

    # ---- occlusion rays generated on the device (rtmi_occlusion_hemisphere*, rtmi_occlusion_targets*, rtmi_ambient_occlusion*) --------------------
    @staticmethod
    def _occlusion_inputs(hits, view):
        hits = np.ascontiguousarray(hits, np.float64).reshape(-1, _ffi.HIT_REC)
        if view is not None:
            view = np.ascontiguousarray(view, np.float64).reshape(-1, 7)
            if len(view) != len(hits):
                raise ValueError("%d view rays for %d points" % (len(view), len(hits)))
        return hits, view

    def occlusion_hemisphere(self, hits, n_dirs, view=None, first=0, seed=RENDER_SEED, time=0.0, t_min=T_MIN, t_max=T_MAX, precision="f64",
                             return_rays=False):
        """n_dirs cosine-weighted rays from every point of hits [n, HIT_REC] (query_hits' records), generated on the device by the hemisphere rule of
        include/rtmi.h (camera.hemisphere_rays_disk restates it) and put through the any-hit search.  view [n, 7]: the rays that found the points
        -- the new rays leave on their side of the surface and carry their time; None: the normal's side and `time`.  A missed record or a
        non-finite one yields no ray.  -> (flags uint8 [n * n_dirs], counts int32 [n], counters {rays generated, occluded rays}), and the rays
        [n * n_dirs, 7] with return_rays."""
        hits, view = self._occlusion_inputs(hits, view)
        n, m = len(hits), len(hits) * int(n_dirs)
        flags, counts, cnt = np.zeros(max(m, 0), np.uint8), np.zeros(n, np.int32), np.zeros(2, np.uint64)
        rays = np.zeros((max(m, 0), 7), np.float64) if return_rays else None
        check(_ffi.lib().rtmi_occlusion_hemisphere(self.handle, _PRECISION[precision], n, ptr(hits), ptr(view), int(n_dirs), int(first), int(seed),
                                                   float(time), float(t_min), float(t_max), ptr(flags), ptr(counts), ptr(rays), ptr(cnt)))
        return (flags, counts, cnt, rays) if return_rays else (flags, counts, cnt)

    def occlusion_hemisphere_device(self, n_points, hits, n_dirs, view=None, first=0, seed=RENDER_SEED, time=0.0, t_min=T_MIN, t_max=T_MAX,
                                    out_occluded=None, out_count=None, out_rays=None, out_counters=None, precision="f64", stream=None):
        """occlusion_hemisphere on HBM-resident buffers (hits as query_hits_device wrote them; every output may be None); asynchronous,
        render_device's stream semantics"""
        check(_ffi.lib().rtmi_occlusion_hemisphere_device(self.handle, _PRECISION[precision], int(n_points), ptr(hits), ptr(view), int(n_dirs), int(first),
                                                          int(seed), float(time), float(t_min), float(t_max), ptr(out_occluded), ptr(out_count),
                                                          ptr(out_rays), ptr(out_counters), ptr(stream)))

    def occlusion_targets(self, hits, targets, view=None, time=0.0, t_min=T_MIN, t_max=1.0 - T_MIN, precision="f64", return_rays=False):
        """One ray from every point of hits [n, HIT_REC] towards each of targets [k, 3] (lights, observers), generated on the device: origin the point,
        direction target - point, so the default range (0.001, 1 - 0.001) asks "up to the target".  view [n, 7]: only its times are read.
        -> (flags uint8 [n * k], counts int32 [n], counters), and the rays with return_rays."""
        hits, view = self._occlusion_inputs(hits, view)
        targets = np.ascontiguousarray(targets, np.float64).reshape(-1, 3)
        n, k = len(hits), len(targets)
        flags, counts, cnt = np.zeros(n * k, np.uint8), np.zeros(n, np.int32), np.zeros(2, np.uint64)
        rays = np.zeros((n * k, 7), np.float64) if return_rays else None
        check(_ffi.lib().rtmi_occlusion_targets(self.handle, _PRECISION[precision], n, ptr(hits), ptr(view), k, ptr(targets), float(time), float(t_min),
                                                float(t_max), ptr(flags), ptr(counts), ptr(rays), ptr(cnt)))
        return (flags, counts, cnt, rays) if return_rays else (flags, counts, cnt)

    def occlusion_targets_device(self, n_points, hits, n_targets, targets, view=None, time=0.0, t_min=T_MIN, t_max=1.0 - T_MIN, out_occluded=None,
                                 out_count=None, out_rays=None, out_counters=None, precision="f64", stream=None):
        """occlusion_targets on HBM-resident buffers; asynchronous, render_device's stream semantics"""
        check(_ffi.lib().rtmi_occlusion_targets_device(self.handle, _PRECISION[precision], int(n_points), ptr(hits), ptr(view), int(n_targets), ptr(targets),
                                                       float(time), float(t_min), float(t_max), ptr(out_occluded), ptr(out_count), ptr(out_rays),
                                                       ptr(out_counters), ptr(stream)))

    def ambient_occlusion_device(self, nx, ny, n_dirs, radius, seed=RENDER_SEED, first=0, precision="f64", out_visibility=None, out_count=None,
                                 out_hits=None, out_counters=None, stream=None):
        """Ambient occlusion of the view, the whole pass on the device (rtmi_ambient_occlusion*): first hits of the pixel-centre rays, n_dirs rays per
        hit by the hemisphere rule on the viewer's side, t-range (0.001, radius), visibility = 1 - occluded / n_dirs and 1 where the primary ray
        missed -- no ray is downloaded, built on the host or uploaded.  The same estimate as ambient_occlusion from other directions (the disk
        sampler's, not the angle's).  Without out_visibility: the host form -> [ny, nx] float64, row 0 = top.  With it (HBM-resident buffers;
        out_count int32 [ny * nx], out_hits [ny * nx, HIT_REC] and out_counters may be None): asynchronous on `stream`, returns None.  first:
        directions [first, first + n_dirs) -- a caller accumulates out_count over calls."""
        if out_visibility is None:
            vis = np.zeros((max(ny, 0), max(nx, 0)), np.float64)
            check(_ffi.lib().rtmi_ambient_occlusion(self.handle, _PRECISION[precision], int(nx), int(ny), int(n_dirs), int(first), float(radius), int(seed),
                                                    ptr(vis), ptr(out_count), ptr(out_hits), ptr(out_counters)))
            return vis
        check(_ffi.lib().rtmi_ambient_occlusion_device(self.handle, _PRECISION[precision], int(nx), int(ny), int(n_dirs), int(first), float(radius), int(seed),
                                                       ptr(out_visibility), ptr(out_count), ptr(out_hits), ptr(out_counters), ptr(stream)))
        return None

    # ---- direct lighting from first hits: the scene's area lights sampled on the device (rtmi_scene_lights, rtmi_direct_irradiance*, rtmi_render_direct*)
    def lights(self):
        """The primitives a light sample can be placed on, in primitive order (int32): spheres and axis-aligned rectangles without a Translate /
        RotateY chain whose material is a DiffuseLight over a Constant texture.  Read from the tables the scene keeps: it follows set_materials
        and set_geometry.  Moving, triangle, instanced, gradient and image emitters are not lights for these calls (they still occlude and show)."""
        count = C.c_int32()
        check(_ffi.lib().rtmi_scene_lights(self.handle, 0, None, C.byref(count)))
        prims = np.zeros(count.value, np.int32)
        check(_ffi.lib().rtmi_scene_lights(self.handle, len(prims), ptr(prims), C.byref(count)))
        return prims

    def _direct_lights(self, lights):
        """-> (the int32 list or None = all eligible, its length, the lights the call will sample)"""
        if lights is None:
            return None, 0, len(self.lights())
        lights = np.ascontiguousarray(lights, np.int32).reshape(-1)
        n = len(lights)
        return (lights if n else np.zeros(1, np.int32)), n, n  # (an empty list is still a list: its pointer must not be NULL)

    def direct_irradiance(self, hits, n_samples, view=None, lights=None, first=0, seed=RENDER_SEED, time=0.0, lambert_only=False, state=None,
                          precision="f64", return_items=False):
        """The direct irradiance at every point of hits [n, HIT_REC] (query_hits' records): n_samples points on each light (lights: primitive
        indices out of self.lights(); None: all of them), one shadow ray each, weighted by both cosines, the inverse square and the light's area
        -- the light rule of include/rtmi.h, which camera.light_samples restates.  view [n, 7]: the rays that found the points (they pick the
        side and the time).  lambert_only: only points on a Lambertian material are lit.  state ([n, DIRECT_REC] float64, updated in place;
        first = 0 starts it, first > 0 continues it): the estimate is then over all samples so far, and any split gives the bits of one call.
        -> (E [n, 3], counters {rays built, occluded rays}); with return_items also the per-item contributions [items, 3], flags uint8 [items]
        and rays [items, 7], item (g * n_samples + k) * n_lights + l."""
        hits, view = self._occlusion_inputs(hits, view)
        lights, n_listed, n_lights = self._direct_lights(lights)
        n = len(hits)
        items = n * max(int(n_samples), 0) * n_lights
        if state is not None and (not isinstance(state, np.ndarray) or state.dtype != np.float64 or not state.flags.c_contiguous
                                  or state.shape != (n, _ffi.DIRECT_REC)):
            raise ValueError("state must be a C-contiguous float64 array [n_points, %d]" % _ffi.DIRECT_REC)
        E, cnt = np.zeros((n, 3), np.float64), np.zeros(2, np.uint64)
        contrib, flags, rays = ((np.zeros((items, 3), np.float64), np.zeros(items, np.uint8), np.zeros((items, 7), np.float64)) if return_items
                                else (None, None, None))
        check(_ffi.lib().rtmi_direct_irradiance(self.handle, _PRECISION[precision], n, ptr(hits), ptr(view), n_listed, ptr(lights), int(n_samples),
                                                int(first), int(seed), float(time), int(bool(lambert_only)), ptr(state), ptr(E), ptr(contrib), ptr(flags),
                                                ptr(rays), ptr(cnt)))
        return (E, cnt, contrib, flags, rays) if return_items else (E, cnt)

    def direct_irradiance_device(self, n_points, hits, n_samples, out_irradiance, view=None, lights=None, first=0, seed=RENDER_SEED, time=0.0,
                                 lambert_only=False, state=None, out_contrib=None, out_occluded=None, out_rays=None, out_counters=None,
                                 precision="f64", stream=None):
        """direct_irradiance on HBM-resident buffers (hits as query_hits_device wrote them; lights stays a host list); asynchronous,
        render_device's stream semantics.  A state's sample count is the caller's contract: it is not read back."""
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        check(_ffi.lib().rtmi_direct_irradiance_device(self.handle, _PRECISION[precision], int(n_points), ptr(hits), ptr(view), n_listed, ptr(lights),
                                                       int(n_samples), int(first), int(seed), float(time), int(bool(lambert_only)), ptr(state),
                                                       ptr(out_irradiance), ptr(out_contrib), ptr(out_occluded), ptr(out_rays), ptr(out_counters),
                                                       ptr(stream)))

    def render_direct(self, nx, ny, n_samples, first=0, seed=RENDER_SEED, state=None, precision="f64", return_hits=False):
        """The view lit directly, the whole pass on the device (rtmi_render_direct): first hits of the pixel-centre rays, n_samples shadow rays per
        hit and eligible light, then per pixel: an emitter shows its emission, a Lambertian surface albedo * E / pi, anything else and a miss is
        black (specular transport is not direct light).  state ([ny * nx, DIRECT_REC], in place) continues the estimate over calls through `first`.
        -> (linear [ny, nx, 3], rgb8 [ny, nx, 3], counters {shadow rays built, occluded}), and the first-hit records [ny * nx, HIT_REC] with
        return_hits; row 0 = top."""
        n = max(nx, 0) * max(ny, 0)
        lin, rgb8, cnt = np.zeros((max(ny, 0), max(nx, 0), 3), np.float64), np.zeros((max(ny, 0), max(nx, 0), 3), np.uint8), np.zeros(2, np.uint64)
        hits = np.zeros((n, _ffi.HIT_REC), np.float64) if return_hits else None
        if state is not None and (not isinstance(state, np.ndarray) or state.dtype != np.float64 or not state.flags.c_contiguous
                                  or state.shape != (n, _ffi.DIRECT_REC)):
            raise ValueError("state must be a C-contiguous float64 array [ny * nx, %d]" % _ffi.DIRECT_REC)
        check(_ffi.lib().rtmi_render_direct(self.handle, _PRECISION[precision], int(nx), int(ny), int(n_samples), int(first), int(seed), ptr(state), ptr(lin),
                                            ptr(rgb8), ptr(hits), ptr(cnt)))
        return (lin, rgb8, cnt, hits) if return_hits else (lin, rgb8, cnt)

    def render_direct_device(self, nx, ny, n_samples, out_linear, out_rgb8=None, out_hits=None, out_counters=None, first=0, seed=RENDER_SEED, state=None,
                             precision="f64", stream=None):
        """render_direct on HBM-resident buffers (out_linear float64 [ny * nx, 3]; the others may be None); asynchronous on `stream`"""
        check(_ffi.lib().rtmi_render_direct_device(self.handle, _PRECISION[precision], int(nx), int(ny), int(n_samples), int(first), int(seed), ptr(state),
                                                   ptr(out_linear), ptr(out_rgb8), ptr(out_hits), ptr(out_counters), ptr(stream)))

    # ---- probes ------------------------------------------------------------------------------------------
    def probe_hit(self, rays, t_min=T_MIN, t_max=T_MAX, precision="f64"):
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 7)
        out = np.zeros((len(rays), 11), np.float64)
        check(_ffi.lib().rtmi_probe_hit(self.handle, _PRECISION[precision], len(rays), ptr(rays), t_min, t_max, ptr(out)))
        return out

    def probe_paths(self, rays, keys, depth=DEFAULT_DEPTH, ctr0=0, max_seg=0, precision="f64"):
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 7)
        keys = np.ascontiguousarray(keys, np.uint64)
        n = len(rays)
        rgb, nseg, nlog = np.zeros((n, 3)), np.zeros(n, np.uint64), np.zeros(n, np.int32)
        log = np.zeros((n, max_seg, _ffi.SEG_REC)) if max_seg else None
        check(_ffi.lib().rtmi_probe_paths(self.handle, _PRECISION[precision], n, ptr(rays), ptr(keys), ctr0, depth,
                                          ptr(rgb), ptr(nseg), ptr(log), max_seg, ptr(nlog)))
        return rgb, nseg, log, nlog

    def probe_paths_nee(self, rays, keys, lights=None, depth=DEFAULT_DEPTH, ctr0=0, max_seg=0, precision="f64"):
        """probe_paths for light-sampled paths (rtmi_probe_paths_nee) -> (rgb [n, 3], segment counts, log [n, max_seg, NEE_REC] or None, logged
        vertices per path, dropped int32 [n] = 1 where the closing emission was dropped).  A log row: SEG_REC's twelve values, the light-sample
        state (0 none, 1 unoccluded, 2 occluded, 3 no ray), the light, d, w, T and the contribution added."""
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 7)
        keys = np.ascontiguousarray(keys, np.uint64)
        n = len(rays)
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        rgb, nseg, nlog, dropped = np.zeros((n, 3)), np.zeros(n, np.uint64), np.zeros(n, np.int32), np.zeros(n, np.int32)
        log = np.zeros((n, max_seg, _ffi.NEE_REC)) if max_seg else None
        check(_ffi.lib().rtmi_probe_paths_nee(self.handle, _PRECISION[precision], n, ptr(rays), ptr(keys), ctr0, depth, n_listed, ptr(lights),
                                              ptr(rgb), ptr(nseg), ptr(dropped), ptr(log), max_seg, ptr(nlog)))
        return rgb, nseg, log, nlog, dropped

    def probe_paths_mis(self, rays, keys, lights=None, light_choice=0, depth=DEFAULT_DEPTH, ctr0=0, max_seg=0, precision="f64"):
        """probe_paths_nee for the MIS rule (rtmi_probe_paths_mis) -> (rgb [n, 3], segment counts, log [n, max_seg, MIS_REC] or None, logged vertices
        per path, weight float64 [n] = the factor on the closing emission, 1 where it is kept whole).  A log row: NEE_REC's twenty-four values, then
        x, m, g of the vertex' light sample and, on a closing vertex whose emission was weighted, x'."""
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 7)
        keys = np.ascontiguousarray(keys, np.uint64)
        n = len(rays)
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        rgb, nseg, nlog, weight = np.zeros((n, 3)), np.zeros(n, np.uint64), np.zeros(n, np.int32), np.zeros(n, np.float64)
        log = np.zeros((n, max_seg, _ffi.MIS_REC)) if max_seg else None
        check(_ffi.lib().rtmi_probe_paths_mis(self.handle, _PRECISION[precision], n, ptr(rays), ptr(keys), ctr0, depth, n_listed, ptr(lights),
                                              self._light_choice(light_choice), ptr(rgb), ptr(nseg), ptr(weight), ptr(log), max_seg, ptr(nlog)))
        return rgb, nseg, log, nlog, weight

    def probe_paths_ris(self, rays, keys, lights=None, depth=DEFAULT_DEPTH, ctr0=0, max_seg=0, precision="f64"):
        """probe_paths_mis for the proposal rule (rtmi_probe_paths_ris) -> (rgb [n, 3], segment counts, log [n, max_seg, RIS_REC] or None, logged
        vertices per path, weight float64 [n] = the factor on the closing emission).  A log row: MIS_REC's twenty-eight values for the chosen
        candidate, then S, w^ of the chosen candidate, r = S / w^ and the number of live candidates."""
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 7)
        keys = np.ascontiguousarray(keys, np.uint64)
        n = len(rays)
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        rgb, nseg, nlog, weight = np.zeros((n, 3)), np.zeros(n, np.uint64), np.zeros(n, np.int32), np.zeros(n, np.float64)
        log = np.zeros((n, max_seg, _ffi.RIS_REC)) if max_seg else None
        check(_ffi.lib().rtmi_probe_paths_ris(self.handle, _PRECISION[precision], n, ptr(rays), ptr(keys), ctr0, depth, n_listed, ptr(lights),
                                              ptr(rgb), ptr(nseg), ptr(weight), ptr(log), max_seg, ptr(nlog)))
        return rgb, nseg, log, nlog, weight

    def probe_paths_vol(self, rays, keys, estimator="mis", lights=None, light_choice=0, depth=DEFAULT_DEPTH, ctr0=0, max_seg=0, precision="f64"):
        """probe_paths_mis for the volume rule (rtmi_probe_paths_vol; estimator "nee" / 1 or "mis" / 2) -> (rgb [n, 3], segment counts, log [n,
        max_seg, VOL_REC] or None, logged vertices per path, weight float64 [n] = the factor on the closing emission; under the NEE rule 0 where it
        is dropped).  A log row: MIS_REC's twenty-eight values (under the NEE rule [21..23] its contribution and [24..27] zeros), then 1.0 where the
        light-sampled vertex is an Isotropic scatter."""
        est = self._vol_estimator(estimator)
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 7)
        keys = np.ascontiguousarray(keys, np.uint64)
        n = len(rays)
        lights, n_listed, _ = (None, 0, 0) if lights is None else self._direct_lights(lights)
        rgb, nseg, nlog, weight = np.zeros((n, 3)), np.zeros(n, np.uint64), np.zeros(n, np.int32), np.zeros(n, np.float64)
        log = np.zeros((n, max_seg, _ffi.VOL_REC)) if max_seg else None
        check(_ffi.lib().rtmi_probe_paths_vol(self.handle, _PRECISION[precision], n, ptr(rays), ptr(keys), ctr0, depth, est,
                                              n_listed, ptr(lights), self._light_choice(light_choice), ptr(rgb), ptr(nseg), ptr(weight), ptr(log),
                                              max_seg, ptr(nlog)))
        return rgb, nseg, log, nlog, weight

    def probe_camera(self, uv, keys, precision="f64"):
        uv = np.ascontiguousarray(uv, np.float64).reshape(-1, 2)
        keys = np.ascontiguousarray(keys, np.uint64)
        out = np.zeros((len(uv), 8))
        check(_ffi.lib().rtmi_probe_camera(self.handle, _PRECISION[precision], len(uv), ptr(uv), ptr(keys), ptr(out)))
        return out

    def probe_texture(self, tex, uvp, precision="f64"):
        uvp = np.ascontiguousarray(uvp, np.float64).reshape(-1, 5)
        out = np.zeros((len(uvp), 3))
        check(_ffi.lib().rtmi_probe_texture(self.handle, _PRECISION[precision], int(tex), len(uvp), ptr(uvp), ptr(out)))
        return out

    def probe_scatter(self, mat, rays, hits, keys, precision="f64"):
        rays = np.ascontiguousarray(rays, np.float64).reshape(-1, 7)
        hits = np.ascontiguousarray(hits, np.float64).reshape(-1, 8)
        keys = np.ascontiguousarray(keys, np.uint64)
        out = np.zeros((len(rays), 9))
        check(_ffi.lib().rtmi_probe_scatter(self.handle, _PRECISION[precision], int(mat), len(rays), ptr(rays), ptr(hits),
                                            ptr(keys), ptr(out)))
        return out


class TemporalAccumulator:
    """Frames of a moving camera that build on each other: every step renders ns samples of the new view and blends the previous result into it
    where the previous view saw the same surface (Context.reproject_device).  The history -- colour, accumulated samples, standard error, the
    features and the camera of the last view -- stays in HBM (torch tensors on the scene's device).
    step(camera) queues, on one stream (stream=: a hipStream_t handle or torch stream; default the context's own) and with ONE synchronisation at
    its end: the stream form of set_camera,
    render_progressive_device(s_first = 0, s_count = ns), render_features_device(na), reproject_device and, with denoise= (True for the library's
    defaults or a dict of Context.denoise_device's iterations / sigma_* arguments), denoise_device of the OUTPUT with its standard error and the
    new features; the history is never filtered.  Step k renders with seed + k: with one seed a still camera would add the same samples again.
    The first step, reset() and a step with another nx, ny or precision start without history.  The context's progressive frame is used.
    Limits: depth is the mean over jittered feature samples, so silhouette pixels are approximate; shading that depends on the view (metal, glass)
    and anything that moves is held back by max_history alone; pixels whose coverage is not 1 never take history."""

    def __init__(self, scene, nx, ny, ns, na=FEATURE_SAMPLES, max_history=REPROJECT_MAX_HISTORY, sigma_d=REPROJECT_SIGMA_D,
                 sigma_n=REPROJECT_SIGMA_N, sigma_a=REPROJECT_SIGMA_A, denoise=None, depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", stream=None):
        if nx <= 0 or ny <= 0 or ns <= 0 or na <= 0:
            raise ValueError("nx, ny, ns and na must be > 0")
        self.scene, self.ns, self.na = scene, int(ns), int(na)
        self.max_history, self.sigma_d, self.sigma_n, self.sigma_a = float(max_history), float(sigma_d), float(sigma_n), float(sigma_a)
        self.denoise = None if denoise is None or denoise is False else ({} if denoise is True else dict(denoise))
        self.depth, self.seed = depth, int(seed)
        self.stream = 0 if stream is None else int(getattr(stream, "cuda_stream", stream))  # 0: the context's own stream
        self.nx = self.ny = self.precision = None
        self._shape(int(nx), int(ny), precision)

    def _shape(self, nx, ny, precision):
        import torch
        dev = torch.device("cuda", self.scene.ctx.device)
        f64 = dict(dtype=torch.float64, device=dev)
        self.nx, self.ny, self.precision = nx, ny, precision
        # two sets of history planes (a step reads one and writes the other), the current frame, the 8-bit frames, the filtered output
        self._lin = [torch.empty((ny, nx, 3), **f64) for _ in range(2)]
        self._w = [torch.empty((ny, nx), **f64) for _ in range(2)]
        self._se = [torch.empty((ny, nx), **f64) for _ in range(2)]
        self._ft = [torch.empty((ny, nx, _ffi.FEATURES), **f64) for _ in range(2)]
        self._cur_lin, self._cur_se = torch.empty((ny, nx, 3), **f64), torch.empty((ny, nx), **f64)
        self._raw_q, self._q = (torch.empty((ny, nx, 3), dtype=torch.uint8, device=dev) for _ in range(2))
        self._cnt = torch.zeros(4, dtype=torch.int64, device=dev)  # {pixels, pixels with history}, {rays, pixels} of the render
        if self.denoise is not None:
            self._dn = (torch.empty((ny, nx, 3), **f64), torch.empty((ny, nx, 3), dtype=torch.uint8, device=dev), torch.empty((ny, nx), **f64))
        self.reset()

    def reset(self):
        """forget the history: the next step returns its own frame (the seed sequence goes on)"""
        self._cam, self._cur = None, 0
        self.steps = getattr(self, "steps", 0)
        self.raw_rgb8 = self.accumulated = None

    def step(self, camera, nx=None, ny=None, precision=None, materials=None, geometry=None):
        """-> (linear [ny,nx,3], rgb8, stderr [ny,nx], weight [ny,nx] = samples behind every pixel, share of the pixels that took history): device
        tensors owned by the accumulator -- rgb8 is overwritten by the next step, the others by the one after it -- filtered if denoise= was
        given (then .accumulated holds the unfiltered four).  .raw_rgb8 is the 8-bit frame of this view's ns samples alone, .rays its
        {total-rays, total-pixels}.
        materials= (a FlatScene or scene, as DeviceScene.set_materials takes it) edits the scene's materials in stream order before this frame
        (the stream form: an edit that would rebuild raises RtmiError -3 before anything is queued).  Such a step starts WITHOUT history
        (share 0), like the first: the colours accumulated so far describe other surfaces.  The step after it takes history again.
        geometry= (as DeviceScene.set_geometry takes it, mode "auto") moves the scene's primitives before this frame; that step starts without
        history too: the reprojection assumes a static world."""
        import torch
        nx, ny, precision = nx or self.nx, ny or self.ny, precision or self.precision
        if (nx, ny, precision) != (self.nx, self.ny, self.precision):
            self._shape(int(nx), int(ny), precision)
        ds, ctx, dev = self.scene, self.scene.ctx, torch.device("cuda", self.scene.ctx.device)
        cam_pair = _camera_pair(camera)
        old, new = self._cur, 1 - self._cur
        first = self._cam is None or materials is not None or geometry is not None
        if first:
            self._w[new].fill_(float(self.ns))
        torch.cuda.synchronize(dev)  # (the allocator or the fill ran on torch's stream; nothing of torch's is queued after this)
        seed = self.seed + self.steps
        lin, se = (self._lin[new], self._se[new]) if first else (self._cur_lin, self._cur_se)
        st = self.stream or None
        if geometry is not None:
            ds.set_geometry(geometry)  # the refit is queued on the context's stream ...
            ds.set_camera(cam_pair)    # ... which the camera's host form waits for: this frame may render on another stream
        if materials is not None:
            ds.set_materials(materials, stream=self.stream)
        ds.set_camera(cam_pair, stream=self.stream)
        ds.render_progressive_device(nx, ny, 0, self.ns, lin, self._raw_q, se, self._cnt[2:], self.depth, seed, precision, st)
        ds.render_features_device(nx, ny, self.na, self._ft[new], None, seed, precision, st)
        if not first:
            ctx.reproject_device(nx, ny, self._cam, cam_pair, self._lin[old], self._w[old], self._se[old], self._ft[old], lin, se, self._ft[new],
                                 float(self.ns), self._lin[new], self._q, self._w[new], self._se[new], self._cnt[:2], self.max_history,
                                 self.sigma_d, self.sigma_n, self.sigma_a, st)
        q = self._raw_q if first else self._q
        self.accumulated = (self._lin[new], q, self._se[new], self._w[new])
        out = self.accumulated
        if self.denoise is not None:
            ctx.denoise_device(nx, ny, self._lin[new], self._se[new], self._ft[new], self._dn[0], self._dn[1], self._dn[2], stream=st, **self.denoise)
            out = (self._dn[0], self._dn[1], self._dn[2], self._w[new])
        torch.cuda.synchronize(dev)
        cnt = self._cnt.cpu().numpy().astype(np.uint64)
        self.rays = cnt[2:]
        self.raw_rgb8 = self._raw_q
        self._cam, self._cur = cam_pair, new
        self.steps += 1
        share = 0.0 if first else float(cnt[1]) / float(cnt[0])
        return out[0], out[1], out[2], out[3], share


def probe_rng(key, d0, n, precision="f64", ctx=None):
    ctx = ctx or default_context()
    bits, real = np.zeros(n, np.uint64), np.zeros(n, np.float64)
    check(_ffi.lib().rtmi_probe_rng(ctx.handle, _PRECISION[precision], key, d0, n, ptr(bits), ptr(real)))
    return bits, real


def probe_arith(abc, ctx=None):
    ctx = ctx or default_context()
    abc = np.ascontiguousarray(abc, np.float64).reshape(-1, 3)
    out = np.zeros_like(abc)
    check(_ffi.lib().rtmi_probe_arith(ctx.handle, len(abc), ptr(abc), ptr(out)))
    return out


def probe_math(abc, tmin=0.001, tmax=3.4028234663852886e38, ctx=None):
    """[n, 12]: sqrt(a), atan2(a, b), asin(a), sphere u, v of (a, b, c), a / b by the per-ray reciprocal, a / (2 pi), reciprocal path taken,
    the traversal's float upper bound of c, the medium's log(a), a / b by the refined reciprocal of a signed divisor, that path taken"""
    ctx = ctx or default_context()
    abc = np.ascontiguousarray(abc, np.float64).reshape(-1, 3)
    slots = 12
    out = np.zeros((len(abc), slots))
    check(_ffi.lib().rtmi_probe_math2(ctx.handle, len(abc), ptr(abc), tmin, tmax, slots, ptr(out)))
    return out


def sample_key(seed, pixel, sample):
    return int(_ffi.lib().rtmi_sample_key(seed, pixel, sample))


# ---- protocol entry points ------------------------------------------------------------------------------
_dummy_camera = None


def _one_off(world_items, camera=None):
    global _dummy_camera
    if camera is None:
        if _dummy_camera is None:
            _dummy_camera = cam.PinholeCamera(np.zeros(3), np.zeros(3), np.zeros(3), np.zeros(3))
        camera = _dummy_camera
    return DeviceScene(hitm.Hitlist(list(world_items)), camera)


def _ray7(r):
    return np.concatenate([np.asarray(r["origin"], np.float64), np.asarray(r["direction"], np.float64), [float(r["time"])]])


def hit(obj, r, t_min, t_max):
    """(hit? obj r t-min t-max) -> {:t :p :uv :normal :material} or None (hitable.clj:7-10), evaluated on the device."""
    items = [obj] if not isinstance(obj, (list, tuple)) else obj
    ds = _one_off(items)
    try:
        o = ds.probe_hit(_ray7(r), float(t_min), float(t_max))[0]
        leaves = []
        fl._leaves(items, leaves, set())
    finally:
        ds.close()
    if o[0] == 0:
        return None
    return {"t": o[2], "p": o[3:6].copy(), "uv": (o[9], o[10]), "normal": o[6:9].copy(), "material": leaves[int(o[1])][0].material}


class _Holder(hitm.Sphere):
    pass


def scatter(material, ray_in, hrec, key=0):
    """(scatter material ray-in hrec) -> {:scattered ray :attenuation vec3} or None (shader.clj:22-24); the draws the
    reference takes from (rand) come from stream `key`."""
    ds = _one_off([hitm.Sphere(np.zeros(3), 1.0, material)])
    try:
        uv = hrec.get("uv", (0.0, 0.0))
        h = np.concatenate([np.asarray(hrec["p"], np.float64), np.asarray(hrec["normal"], np.float64), [uv[0], uv[1]]])
        o = ds.probe_scatter(0, _ray7(ray_in), h, np.array([key], np.uint64))[0]
    finally:
        ds.close()
    if o[0] == 0:
        return None
    return {"scattered": {"origin": np.asarray(hrec["p"], np.float64), "direction": o[1:4].copy(), "time": o[7]},
            "attenuation": o[4:7].copy()}


def emitted(material, uv, p):
    """(emitted material uv p) (shader.clj:22-24): zero except DiffuseLight = (sample tex uv p)."""
    if isinstance(material, shad.DiffuseLight):
        return sample(material.tex, uv, p)
    return np.zeros(3)


def sample(tex, uv, p):
    """(sample tex uv p) (texture.clj:8-9), evaluated on the device."""
    ds = _one_off([hitm.Sphere(np.zeros(3), 1.0, shad.Lambertian(tex))])
    try:
        t = int(ds.flat.mat_tex[0])
        return ds.probe_texture(t, np.concatenate([[uv[0], uv[1]], np.asarray(p, np.float64)]))[0]
    finally:
        ds.close()


def get_ray(camera, u, v, key=0):
    """(get-ray camera u v) (camera.clj:5-6), evaluated on the device; lens/time draws come from stream `key`."""
    ds = _one_off([], camera)
    try:
        o = ds.probe_camera(np.array([u, v], np.float64), np.array([key], np.uint64))[0]
    finally:
        ds.close()
    return {"origin": o[0:3].copy(), "direction": o[3:6].copy(), "time": o[6]}


# ---- driver --------------------------------------------------------------------------------------------
def render(scene, nx, ny, ns, depth=DEFAULT_DEPTH, seed=RENDER_SEED, precision="f64", ctx=None):
    """Render {:camera :world} -> (linear, rgb8, counters).  Replaces core.clj:100-108."""
    ds = DeviceScene(scene, ctx=ctx)
    try:
        return ds.render(nx, ny, ns, depth, seed, precision)
    finally:
        ds.close()


def save_ppm(path, rgb8):
    """imagez `save` (core.clj:112) has no PPM writer; binary P6 written here."""
    h, w, _ = rgb8.shape
    with open(path, "wb") as f:
        f.write(b"P6\n%d %d\n255\n" % (w, h))
        f.write(np.ascontiguousarray(rgb8, np.uint8).tobytes())


def save_png(path, rgb8):
    """imagez `save` (core.clj:112) writes whatever the extension says, PNG by default (core.clj:76): 8-bit RGB, no alpha,
    one zlib stream, filter 0 on every row (stdlib only)."""
    import struct
    import zlib
    a = np.ascontiguousarray(rgb8, np.uint8)
    h, w, _ = a.shape
    raw = np.concatenate([np.zeros((h, 1), np.uint8), a.reshape(h, w * 3)], axis=1).tobytes()

    def chunk(tag, data):
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


SCENES = {  # the scene choices of core.clj:82-90 (there: commented-out lines; here: the 5th argument)
    "random": lambda s, nx, ny: s.make_random_scene(nx, ny, 11, True),      # core.clj:89, the Shirley cover scene
    "final": lambda s, nx, ny: s.make_final(nx, ny),                        # core.clj:90, the line that is active as shipped
    "two-spheres": lambda s, nx, ny: s.make_two_spheres(nx, ny),            # core.clj:82
    "two-perlin-spheres": lambda s, nx, ny: s.make_two_perlin_spheres(nx, ny),
    "textured-sphere": lambda s, nx, ny: s.make_textured_sphere(nx, ny),
    "subsurface-sphere": lambda s, nx, ny: s.make_subsurface_sphere(nx, ny),
    "two-triangles": lambda s, nx, ny: s.make_two_triangles(nx, ny),
    "example-light": lambda s, nx, ny: s.make_example_light(nx, ny),
    "cornell-box": lambda s, nx, ny: s.make_cornell_box(nx, ny, False),     # core.clj:88 passes classic = false
    "cornell-box-classic": lambda s, nx, ny: s.make_cornell_box(nx, ny, True),
}


def _progressive_flags(argv):
    """-> (positional arguments, chunk, budget, noise, adaptive): the optional flags --chunk K, --budget SECONDS, --noise EPS, --adaptive EPS,
    checked here, before any device work (None when absent)"""
    import math
    rest, flags = [], {}
    conv = {"--chunk": int, "--budget": float, "--noise": float, "--adaptive": float}
    i = 0
    while i < len(argv):
        a = argv[i]
        key, val = (a.split("=", 1) + [None])[:2] if a.startswith("--") else (a, None)
        if key not in conv:
            rest.append(a)
            i += 1
            continue
        if val is None:
            if i + 1 >= len(argv):
                raise SystemExit("%s needs a value" % key)
            val = argv[i + 1]
            i += 1
        i += 1
        try:
            v = conv[key](val)
        except ValueError:
            raise SystemExit("%s %r is not a number" % (key, val))
        if key == "--chunk" and v <= 0:
            raise SystemExit("--chunk must be a positive number of samples (got %d)" % v)
        if key != "--chunk" and not (math.isfinite(v) and v >= 0):
            raise SystemExit("%s must be a finite number >= 0 (got %r)" % (key, val))
        flags[key] = v
    if "--adaptive" in flags and "--noise" in flags:
        raise SystemExit("--adaptive and --noise are two stopping rules: give one of them")
    return rest, flags.get("--chunk"), flags.get("--budget"), flags.get("--noise"), flags.get("--adaptive")


def _denoise_flags(argv):
    """-> (the other arguments, iterations, feature samples): --denoise [ITERATIONS] (an integer right after it, or --denoise=K, is its value;
    default DENOISE_ITERATIONS) and --feature-samples N, checked here, before any device work (None when absent)"""
    import re
    rest, iterations, na = [], None, None
    i = 0
    while i < len(argv):
        a = argv[i]
        key, val = (a.split("=", 1) + [None])[:2] if a.startswith("--") else (a, None)
        i += 1
        if key == "--denoise":
            if val is None and i < len(argv) and re.fullmatch(r"[+-]?[0-9]+", argv[i]):
                val = argv[i]
                i += 1
            try:
                iterations = DENOISE_ITERATIONS if val is None else int(val)
            except ValueError:
                raise SystemExit("--denoise %r is not a number of passes" % val)
            if not 0 <= iterations <= 8:
                raise SystemExit("--denoise takes 0 to 8 passes (got %d)" % iterations)
        elif key == "--feature-samples":
            if val is None:
                if i >= len(argv):
                    raise SystemExit("--feature-samples needs a value")
                val = argv[i]
                i += 1
            try:
                na = int(val)
            except ValueError:
                raise SystemExit("--feature-samples %r is not a number" % val)
            if na <= 0:
                raise SystemExit("--feature-samples must be a positive number of samples (got %d)" % na)
        else:
            rest.append(a)
    if na is not None and iterations is None:
        raise SystemExit("--feature-samples belongs to --denoise")
    return rest, iterations, na


def _adaptive_denoised_flags(argv):
    """-> (the other arguments, eps): --adaptive-denoised EPS, checked here, before any device work (None when absent).  It is a stopping rule
    of its own: it does not combine with --adaptive or --noise."""
    import math
    rest, eps = [], None
    i = 0
    while i < len(argv):
        a = argv[i]
        key, val = (a.split("=", 1) + [None])[:2] if a.startswith("--") else (a, None)
        i += 1
        if key != "--adaptive-denoised":
            rest.append(a)
            continue
        if val is None:
            if i >= len(argv):
                raise SystemExit("--adaptive-denoised needs a value")
            val = argv[i]
            i += 1
        try:
            eps = float(val)
        except ValueError:
            raise SystemExit("--adaptive-denoised %r is not a number" % val)
        if not (math.isfinite(eps) and eps >= 0):
            raise SystemExit("--adaptive-denoised must be a finite number >= 0 (got %r)" % val)
    if eps is not None:
        for other in ("--adaptive", "--noise"):
            if any(a.split("=", 1)[0] == other for a in rest):
                raise SystemExit("--adaptive-denoised and %s are two stopping rules: give one of them" % other)
    return rest, eps


def _orbit_flags(argv):
    """-> (the other arguments, views): --orbit N, checked here, before any device work (None when absent).  An orbit is a set of one-shot
    frames of one live scene: it combines with --denoise and with none of the progressive / adaptive modes."""
    rest, views = [], None
    i = 0
    while i < len(argv):
        a = argv[i]
        key, val = (a.split("=", 1) + [None])[:2] if a.startswith("--") else (a, None)
        i += 1
        if key != "--orbit":
            rest.append(a)
            continue
        if val is None:
            if i >= len(argv):
                raise SystemExit("--orbit needs a value")
            val = argv[i]
            i += 1
        try:
            views = int(val)
        except ValueError:
            raise SystemExit("--orbit %r is not a number of views" % val)
        if views <= 0:
            raise SystemExit("--orbit must be a positive number of views (got %d)" % views)
    if views is not None:
        for other in ("--chunk", "--budget", "--noise", "--adaptive", "--adaptive-denoised"):
            if any(a.split("=", 1)[0] == other for a in rest):
                raise SystemExit("--orbit renders one-shot frames: it does not combine with %s" % other)
    return rest, views


def _accumulate_flags(argv, orbit_views=None):
    """-> (the other arguments, max_history): --accumulate [MAX_HISTORY] (a number right after it, or --accumulate=M, is its value; "inf" = no cap;
    default REPROJECT_MAX_HISTORY), checked here, before any device work (None when absent).  It belongs to --orbit: the views of an orbit build
    on each other."""
    import math
    import re
    rest, cap = [], None
    i = 0
    while i < len(argv):
        a = argv[i]
        key, val = (a.split("=", 1) + [None])[:2] if a.startswith("--") else (a, None)
        i += 1
        if key != "--accumulate":
            rest.append(a)
            continue
        if val is None and i < len(argv) and re.fullmatch(r"[+-]?([0-9]+\.?[0-9]*([eE][+-]?[0-9]+)?|\.[0-9]+|inf|nan)", argv[i]):
            val = argv[i]
            i += 1
        try:
            cap = REPROJECT_MAX_HISTORY if val is None else float(val)
        except ValueError:
            raise SystemExit("--accumulate %r is not a number of samples" % val)
        if math.isnan(cap) or cap <= 0:
            raise SystemExit("--accumulate takes the cap of the history's weight in samples, > 0 or inf (got %r)" % val)
    if cap is not None and orbit_views is None:
        raise SystemExit("--accumulate belongs to --orbit")
    return rest, cap


def _accumulated_name(name):
    """x_007.png -> x_007.acc.png: the accumulated frame is written next to the view's own"""
    import os
    root, ext = os.path.splitext(name)
    return root + ".acc" + ext


def _orbit_name(name, k):
    """x.png -> x_007.png: view k of an orbit"""
    import os
    root, ext = os.path.splitext(name)
    return "%s_%03d%s" % (root, k, ext)


def _render_orbit_accumulated(sc, name, nx, ny, nr, views, dn_iterations, dn_samples, max_history, tstart):
    """--orbit with --accumulate: the views through ONE TemporalAccumulator.  Writes name_000.ext ... (every view's own nr samples; view k is
    rendered with seed RENDER_SEED + k), name_000.acc.ext ... (the accumulated frames) and, with --denoise, name_000.acc.denoised.ext ..."""
    pivot = sc.get("lookat") if isinstance(sc, dict) else None
    ds = DeviceScene(sc)
    rays = pixels = 0
    try:
        dn = None if dn_iterations is None else {"iterations": dn_iterations}
        acc = TemporalAccumulator(ds, nx, ny, nr, na=FEATURE_SAMPLES if dn_samples is None else dn_samples, max_history=max_history, denoise=dn)
        for k, camera in enumerate(cam.orbit(sc["camera"], views, pivot)):
            lin, rgb8, err, weight, share = acc.step(camera)
            _show_progress(tstart, k + 1, views)
            print("history on %.1f%% of the pixels, %.1f samples behind a pixel on average" % (100.0 * share, float(weight.mean())))
            _save_image(_orbit_name(name, k), acc.raw_rgb8.cpu().numpy())
            _save_image(_accumulated_name(_orbit_name(name, k)), acc.accumulated[1].cpu().numpy())
            if dn is not None:
                _save_image(_denoised_name(_accumulated_name(_orbit_name(name, k))), rgb8.cpu().numpy())
            rays, pixels = rays + int(acc.rays[0]), pixels + int(acc.rays[1])
    finally:
        ds.ctx.progressive_release()
        ds.close()
    print("total-rays %d total-pixels %d" % (rays, pixels))  # metrics.clj:8-9, summed over the views
    return 0


def _render_orbit(sc, name, nx, ny, nr, views, dn_iterations, dn_samples, tstart):
    """--orbit: `views` frames of ONE device scene, view k turned by k * 360 / views degrees about the vertical axis through the scene's
    look-at point (sc["lookat"] when the scene gives one, else the centre of the camera's image plane, which lies on the look-at axis);
    only the camera moves between the frames (DeviceScene.set_camera).  Writes name_000.ext ... and, with --denoise, name_000.denoised.ext ..."""
    pivot = sc.get("lookat") if isinstance(sc, dict) else None
    ds = DeviceScene(sc)
    rays = pixels = 0
    try:
        for k, camera in enumerate(cam.orbit(sc["camera"], views, pivot)):
            ds.set_camera(camera)
            if dn_iterations is None:
                lin, rgb8, cnt = ds.render(nx, ny, nr)
            else:
                lin, rgb8, err, cnt = ds.render_progressive(nx, ny, 0, nr)
            _show_progress(tstart, k + 1, views)
            _save_image(_orbit_name(name, k), rgb8)
            if dn_iterations is not None:
                _save_image(_denoised_name(_orbit_name(name, k)), _denoise_frame(ds, nx, ny, lin, err, dn_iterations, dn_samples))
            rays, pixels = rays + int(cnt[0]), pixels + int(cnt[1])
    finally:
        ds.ctx.progressive_release()
        ds.close()
    print("total-rays %d total-pixels %d" % (rays, pixels))  # metrics.clj:8-9, summed over the views
    return 0


def _ao_flags(argv, flag="--ao"):
    """-> (the other arguments, (directions, radius) or None): --ao N [RADIUS] (a number right after N, or --ao=N, is taken; default radius 1.0),
    checked here, before any device work.  flag: the same for --ao-device."""
    import re
    rest, ao = [], None
    number = r"[+]?([0-9]+\.?[0-9]*|\.[0-9]+)([eE][+-]?[0-9]+)?"
    i = 0
    while i < len(argv):
        a = argv[i]
        key, val = (a.split("=", 1) + [None])[:2] if a.startswith("--") else (a, None)
        i += 1
        if key != flag:
            rest.append(a)
            continue
        if val is None:
            if i >= len(argv):
                raise SystemExit("%s needs a number of directions" % flag)
            val = argv[i]
            i += 1
        try:
            n_dirs = int(val)
        except ValueError:
            raise SystemExit("%s %r is not a number of directions" % (flag, val))
        if n_dirs <= 0:
            raise SystemExit("%s takes a positive number of directions (got %d)" % (flag, n_dirs))
        radius = 1.0
        if i < len(argv) and re.fullmatch(number, argv[i]):
            radius = float(argv[i])
            i += 1
        if not radius > 0.0:
            raise SystemExit("%s takes a positive radius (got %g)" % (flag, radius))
        ao = (n_dirs, radius)
    return rest, ao


def _ao_name(name):
    """x.png -> x.ao.png: the visibility map is written next to the frame"""
    import os
    root, ext = os.path.splitext(name)
    return root + ".ao" + ext


def _direct_flags(argv):
    """-> (the other arguments, samples or None): --direct N or --direct=N, checked here, before any device work"""
    rest, samples = [], None
    i = 0
    while i < len(argv):
        a = argv[i]
        key, val = (a.split("=", 1) + [None])[:2] if a.startswith("--") else (a, None)
        i += 1
        if key != "--direct":
            rest.append(a)
            continue
        if val is None:
            if i >= len(argv):
                raise SystemExit("--direct needs a number of samples per light")
            val = argv[i]
            i += 1
        try:
            samples = int(val)
        except ValueError:
            raise SystemExit("--direct %r is not a number of samples" % val)
        if samples <= 0:
            raise SystemExit("--direct takes a positive number of samples (got %d)" % samples)
    return rest, samples


def _nee_flags(argv, panorama=False, orbit=False):
    """-> (the other arguments, whether --nee was given); the modes it does not combine with are refused here, before any device work"""
    rest = [a for a in argv if a != "--nee"]
    given = len(rest) != len(argv)
    for a in rest:
        if a.startswith("--nee"):
            raise SystemExit("--nee takes no value (got %r)" % a)
    if given and (panorama or orbit):
        raise SystemExit("--nee does not combine with --orbit or --panorama")
    return rest, given


def _nee_name(name):
    """x.png -> x.nee.png: the light-sampled frame is written next to the frame"""
    import os
    root, ext = os.path.splitext(name)
    return root + ".nee" + ext


MIS_CHOICES = {"uniform": 0, "power": 1}  # light_choice of the MIS calls


def _mis_flags(argv, panorama=False, orbit=False):
    """-> (the other arguments, None or the light choice of --mis [uniform|power], default uniform); refused where --nee is, before any device work"""
    rest, choice, k = [], None, 0
    while k < len(argv):
        a = argv[k]
        if a == "--mis":
            if choice is not None:
                raise SystemExit("--mis given twice")
            choice = "uniform"
            if k + 1 < len(argv) and argv[k + 1] in MIS_CHOICES:
                choice = argv[k + 1]
                k += 1
        elif a.startswith("--mis"):
            raise SystemExit("--mis takes uniform or power as a separate word (got %r)" % a)
        else:
            rest.append(a)
        k += 1
    if choice is not None and (panorama or orbit):
        raise SystemExit("--mis does not combine with --orbit or --panorama")
    return rest, choice


def _mis_name(name):
    """x.png -> x.mis.png: the frame of the MIS paths is written next to the frame"""
    import os
    root, ext = os.path.splitext(name)
    return root + ".mis" + ext


LIT_ESTIMATORS = {"plain": 0, "nee": 1, "mis": 2}  # estimator of rtmi_render_lit


def _lit_flags(argv, panorama=False, orbit=False, nee=False, mis=False):
    """-> (the other arguments, None or (estimator, light choice) of --lit [plain|nee|mis[:uniform|:power]|ris], default mis; ris: the proposal rule,
    which has no light choice); the modes it does not combine with are refused here, before any device work"""
    rest, lit, k = [], None, 0
    while k < len(argv):
        a = argv[k]
        if a == "--lit":
            if lit is not None:
                raise SystemExit("--lit given twice")
            lit = ("mis", "uniform")
            if k + 1 < len(argv):
                est, _, choice = argv[k + 1].partition(":")
                if est in LIT_ESTIMATORS or est == "ris":
                    if choice and (est != "mis" or choice not in MIS_CHOICES):
                        raise SystemExit("--lit takes plain, nee, mis, mis:uniform, mis:power or ris (got %r)" % argv[k + 1])
                    lit = (est, choice or "uniform")
                    k += 1
        elif a.startswith("--lit"):
            raise SystemExit("--lit takes plain, nee or mis[:power] as a separate word (got %r)" % a)
        else:
            rest.append(a)
        k += 1
    if lit is not None and (panorama or orbit):
        raise SystemExit("--lit does not combine with --orbit or --panorama")
    if lit is not None and (nee or mis):
        raise SystemExit("--lit does not combine with --nee or --mis: it is their frame through the scene's own streams")
    return rest, lit


VOL_ESTIMATORS = {"nee": 1, "mis": 2}  # estimator of the volume rule's calls


def _devices_flags(argv, lit=False):
    """-> (the other arguments, None or the device ordinals of --devices 0,1,...: the light-sampled frame is refined on one replica per listed device
    (dist.MultiDevice; an ordinal may repeat, to rehearse on one GPU)); accepted only together with --lit or --lit-vol"""
    rest, devices, k = [], None, 0
    while k < len(argv):
        a = argv[k]
        if a == "--devices":
            if devices is not None:
                raise SystemExit("--devices given twice")
            words = argv[k + 1].split(",") if k + 1 < len(argv) else []
            if not words or not all(w.isdigit() for w in words):
                raise SystemExit("--devices takes device ordinals separated by commas, as in --devices 0,1 (got %r)" % (argv[k + 1] if k + 1 < len(argv) else ""))
            devices = [int(w) for w in words]
            if len(devices) > 8:
                raise SystemExit("--devices takes at most 8 devices (got %d)" % len(devices))
            k += 1
        elif a.startswith("--devices"):
            raise SystemExit("--devices takes its list as a separate word (got %r)" % a)
        else:
            rest.append(a)
        k += 1
    if devices is not None and not lit:
        raise SystemExit("--devices goes with --lit or --lit-vol: it spreads the light-sampled frame over the listed devices")
    return rest, devices


def _lit_vol_flags(argv, panorama=False, orbit=False, nee=False, mis=False):
    """-> (the other arguments, None or (estimator, light choice) of --lit-vol [nee|mis[:uniform|:power]], default mis); it is taken out of the
    arguments before --lit is looked for, and the modes it does not combine with (--lit among them) are refused here, before any device work"""
    rest, vol, k = [], None, 0
    while k < len(argv):
        a = argv[k]
        if a == "--lit-vol":
            if vol is not None:
                raise SystemExit("--lit-vol given twice")
            vol = ("mis", "uniform")
            if k + 1 < len(argv):
                est, _, choice = argv[k + 1].partition(":")
                if est in VOL_ESTIMATORS:
                    if choice and (est != "mis" or choice not in MIS_CHOICES):
                        raise SystemExit("--lit-vol takes nee, mis, mis:uniform or mis:power (got %r)" % argv[k + 1])
                    vol = (est, choice or "uniform")
                    k += 1
        elif a.startswith("--lit-vol"):
            raise SystemExit("--lit-vol takes nee or mis[:power] as a separate word (got %r)" % a)
        else:
            rest.append(a)
        k += 1
    if vol is not None and (panorama or orbit):
        raise SystemExit("--lit-vol does not combine with --orbit or --panorama")
    if vol is not None and (nee or mis or any(a == "--lit" for a in rest)):
        raise SystemExit("--lit-vol does not combine with --lit, --nee or --mis: it is their frame on a scene that holds a ConstantMedium")
    return rest, vol


def _lit_vol_name(name):
    """x.png -> x.vol.png: the frame of rtmi_render_lit_vol is written next to the frame"""
    import os
    root, ext = os.path.splitext(name)
    return root + ".vol" + ext


def _lit_name(name):
    """x.png -> x.lit.png: the frame of rtmi_render_lit is written next to the frame"""
    import os
    root, ext = os.path.splitext(name)
    return root + ".lit" + ext


def _direct_name(name):
    """x.png -> x.direct.png: the directly lit view is written next to the frame"""
    import os
    root, ext = os.path.splitext(name)
    return root + ".direct" + ext


def _denoised_name(name):
    """x.png -> x.denoised.png: the filtered image is written next to the unfiltered one"""
    import os
    root, ext = os.path.splitext(name)
    return root + ".denoised" + ext


def _denoise_frame(ds, nx, ny, lin, err, iterations, na):
    """the filtered 8-bit frame of a run with --denoise: the features of the frame, then the filter with the default sigmas"""
    ft, _ = ds.render_features(nx, ny, FEATURE_SAMPLES if na is None else na)
    return ds.ctx.denoise(lin, err, ft, iterations=iterations)[1]


def _save_image(name, rgb8):
    if name.lower().endswith(".ppm"):
        save_ppm(name, rgb8)
    elif name.lower().endswith(".npy"):
        np.save(name, rgb8)
    else:
        save_png(name, rgb8)
    print("wrote", name)  # core.clj:113


def _show_progress(tstart, k, ns):
    """display.clj:20-24 after a chunk: elapsed, percent done, ETA"""
    elapsed = time.time() - tstart
    pct = k / ns
    print("%.2fs, %d%%, ETA %.2fs" % (elapsed, int(100.0 * pct), elapsed * (1 - pct) / pct), flush=True)
    return elapsed


def main(argv=None):
    """lein-run compatible: `name nx ny ns [win|scene]` (core.clj:73-80).  The reference picks its scene by editing the
    source (core.clj:82-90); here the 5th argument names it (default: the cover scene; "true"/"win", the reference's
    window switch, is accepted and ignored -- there is no display on this path).
    Optional flags: --chunk K renders the frame progressively in chunks of K samples and prints the reference's progress line
    (display.clj:20-24) after each; --budget SECONDS stops after the first chunk that ends past the budget; --noise EPS stops after the
    first chunk at which 99 % of the pixels have a standard error <= EPS (--budget / --noise alone: chunks of 16).  ns stays the cap; the
    image after k samples is the one-shot render's with ns = k.
    --adaptive EPS samples adaptively instead (refine_adaptive, rounds of --chunk, default 16): an 8x8 tile stops taking samples once all its
    pixels have a standard error <= EPS, and the run ends when no tile is left or at ns; every tile equals the one-shot render with the
    samples it took.  --budget applies; --noise does not combine with it.
    --denoise [ITERATIONS] also writes the frame filtered by the edge-aware denoiser (Context.denoise, default sigmas, ITERATIONS passes, default
    5) next to the unfiltered one, as name.denoised.ext; --feature-samples N sets the samples of its feature buffers (default 4).  It works with
    every mode above; the unfiltered file and the progress lines are what they are without it.
    --adaptive-denoised EPS samples adaptively for a frame that is filtered anyway (refine_adaptive_denoised, rounds of --chunk, default 16):
    after every round the frame is denoised and an 8x8 tile stops taking samples once the FILTERED standard error of all its pixels is <= EPS.
    It writes name.ext unfiltered and name.denoised.ext, prints the "samples: mean ..." line, implies --denoise with the defaults unless
    --denoise / --feature-samples are given, obeys --budget and does not combine with --adaptive or --noise.
    --orbit N renders N one-shot views of the scene, view k turned by k * 360 / N degrees about the vertical axis through the scene's look-at
    point, from ONE device scene whose camera moves between the frames (DeviceScene.set_camera); it writes name_000.ext, name_001.ext, ...,
    works with --denoise (name_000.denoised.ext, ...) and does not combine with the progressive and adaptive modes.
    --accumulate [MAX_HISTORY] belongs to --orbit: the views build on each other (TemporalAccumulator: the previous view's result is reprojected
    into the next camera and blended where both see the same surface; MAX_HISTORY caps the samples a history may count for, default 8, inf =
    no cap).  View k is rendered with seed RENDER_SEED + k; it writes name_000.ext (the view's own samples), name_000.acc.ext (accumulated) and,
    with --denoise, name_000.acc.denoised.ext.
    --panorama renders the full sphere around the scene's camera position as an equirectangular image of 2 ny x ny pixels (nx is ignored): rays
    from camera.panorama_rays through DeviceScene.render_with, ns samples per pixel in chunks of 16.  It does not combine with the other modes.
    --ao N [RADIUS] also writes the view's ambient occlusion (DeviceScene.ambient_occlusion: N cosine-weighted any-hit rays of length RADIUS, default
    1.0, from the first hit under every pixel centre) as a grey image, name.ao.ext, beside the frame.  It does not combine with --orbit or --panorama.
    --ao-device N [RADIUS] writes the same kind of image through DeviceScene.ambient_occlusion_device: the rays are generated on the device (the disk
    sampler's directions, not --ao's: the same estimate from other rays).  It takes the place of --ao.
    --direct N also writes the view lit directly (DeviceScene.render_direct: N shadow rays per first hit towards every area light the scene holds,
    sampled on the device) as name.direct.ext, beside the frame.  It does not combine with --orbit or --panorama.
    --nee also writes the frame traced by light-sampled paths (DeviceScene.render_nee: ns paths per pixel, one shadow ray per Lambertian vertex) as
    name.nee.ext, beside the frame.  It does not combine with --orbit or --panorama, and a scene that holds a ConstantMedium is refused.
    --mis [uniform|power] also writes the frame of those paths under multiple importance sampling (DeviceScene.render_nee(mis=True): the light sample
    and the scatter share each lamp's emission by the balance heuristic; the light is picked uniformly, the default, or by power) as name.mis.ext.
    It is refused where --nee is.
    --lit [plain|nee|mis[:power]] also writes the frame of DeviceScene.render_lit (default mis): the samples the frame itself traces -- the same keys, jitter,
    lens draws and streams, the camera rays built on the device -- under the plain estimator, the NEE rule, the MIS rule or (--lit ris) the proposal
    rule, where every lamp proposes a point at each vertex and one shadow ray is sent (DeviceScene.render_lit_ris), as name.lit.ext.  With --chunk
    K it is refined K samples at a time through one state (the same image).  It does not combine with --orbit, --panorama, --nee or --mis.
    --lit-vol [nee|mis[:power]] also writes the frame of DeviceScene.render_lit_vol (default mis) as name.vol.ext: --lit's frame under the volume rule,
    for the scenes that hold a ConstantMedium (final, the smoke cornell-box, subsurface) -- the vertices inside a medium sample the lights too and the
    shadow rays draw their own way through the media.  With --chunk K it is refined K samples at a time.  It does not combine with --lit, --nee, --mis,
    --orbit or --panorama.
    --lit / --lit-vol with --adaptive EPS (or --adaptive-denoised EPS) refine their frame adaptively too (DeviceScene.refine_lit_adaptive, rounds of
    --chunk): an 8x8 tile stops taking samples once its standard error (its filtered standard error) is <= EPS everywhere, ns is the cap, and a line
    reports the share of the pixel-samples taken.
    --devices 0,1,... refines the frame of --lit / --lit-vol on one replica per listed device (dist.MultiDevice.render_lit / refine_lit_adaptive: the
    8x8 tiles dealt round-robin, one gather per chunk), with or without --chunk, --adaptive or --adaptive-denoised: the same image, bit for bit.  It
    is refused without --lit or --lit-vol."""
    from . import scene as scenes
    argv = list(sys.argv[1:] if argv is None else argv)
    argv, direct = _direct_flags(argv)
    argv, ao = _ao_flags(argv)
    argv, ao_device = _ao_flags(argv, "--ao-device")
    if ao is not None and ao_device is not None:
        raise SystemExit("--ao and --ao-device write the same file: give one of them")
    ao_on_device, ao = ao_device is not None, ao_device if ao_device is not None else ao
    panorama = "--panorama" in argv
    argv = [x for x in argv if x != "--panorama"]
    argv, orbit_views = _orbit_flags(argv)
    if ao is not None and (panorama or orbit_views is not None):
        raise SystemExit("--ao does not combine with --orbit or --panorama")
    if direct is not None and (panorama or orbit_views is not None):
        raise SystemExit("--direct does not combine with --orbit or --panorama")
    argv, nee = _nee_flags(argv, panorama, orbit_views is not None)
    argv, mis = _mis_flags(argv, panorama, orbit_views is not None)
    argv, vol_mode = _lit_vol_flags(argv, panorama, orbit_views is not None, nee, mis is not None)
    argv, lit_mode = _lit_flags(argv, panorama, orbit_views is not None, nee, mis is not None)
    argv, devices = _devices_flags(argv, lit_mode is not None or vol_mode is not None)
    argv, accumulate = _accumulate_flags(argv, orbit_views)
    argv, adaptive_denoised = _adaptive_denoised_flags(argv)
    if adaptive_denoised is not None and not any(a.split("=", 1)[0] == "--denoise" for a in argv):
        argv.append("--denoise")  # implied, with the default passes; --feature-samples then belongs to it
    argv, dn_iterations, dn_samples = _denoise_flags(argv)
    argv, chunk, budget, noise, adaptive = _progressive_flags(argv)
    if panorama and any(x is not None for x in (chunk, budget, noise, adaptive, dn_iterations, orbit_views, accumulate, adaptive_denoised)):
        raise SystemExit("--panorama does not combine with the other modes")
    if chunk is None and (budget is not None or noise is not None or adaptive is not None or adaptive_denoised is not None):
        chunk = 16
    name = argv[0] if len(argv) > 0 else "render.png"  # core.clj:76
    nx = int(argv[1]) if len(argv) > 1 else 200
    ny = int(argv[2]) if len(argv) > 2 else 100
    nr = int(argv[3]) if len(argv) > 3 else 100
    which = argv[4] if len(argv) > 4 and argv[4] not in ("true", "win") else "random"
    if which not in SCENES:
        raise SystemExit("unknown scene %r; one of %s" % (which, ", ".join(sorted(SCENES))))
    tstart = time.time()
    sc = SCENES[which](scenes, nx, ny)
    if (nee or mis is not None) and (fl.flatten(sc).prim_kind & 15 == fl.PRIM_MEDIUM).any():
        raise SystemExit("%s: scene %r holds a ConstantMedium, which the light-sampled paths do not trace" % ("--nee" if nee else "--mis", which))
    if lit_mode is not None and lit_mode[0] != "plain" and (fl.flatten(sc).prim_kind & 15 == fl.PRIM_MEDIUM).any():
        raise SystemExit("--lit %s: scene %r holds a ConstantMedium, which the light-sampled paths do not trace" % (lit_mode[0], which))
    if accumulate is not None:
        return _render_orbit_accumulated(sc, name, nx, ny, nr, orbit_views, dn_iterations, dn_samples, accumulate, tstart)
    if orbit_views is not None:
        return _render_orbit(sc, name, nx, ny, nr, orbit_views, dn_iterations, dn_samples, tstart)
    filtered = None
    if panorama:
        nx = 2 * ny
        camera = sc["camera"]
        ds = DeviceScene(sc)
        try:
            lin, rgb8, err, cnt = ds.render_with(cam.panorama_rays, nx, ny, nr, min(nr, 16), lookfrom=camera.origin, lookat=cam.view_pivot(camera),
                                                 vup=camera.vert)
        finally:
            ds.close()
        cnt = (cnt[0], nx * ny)  # the summary line counts pixels; render_with counts rays
        print("%.2fs, %d%%, ETA %.2fs" % (time.time() - tstart, 100, 0.0))  # display.clj:20-24
    elif chunk is None and dn_iterations is None:
        lin, rgb8, cnt = render(sc, nx, ny, nr)
        elapsed = time.time() - tstart
        print("%.2fs, %d%%, ETA %.2fs" % (elapsed, 100, 0.0))  # display.clj:20-24
    elif chunk is None:  # the one-shot frame through the progressive call: the same image, and the noise estimate the filter reads
        ds = DeviceScene(sc)
        try:
            lin, rgb8, err, cnt = ds.render_progressive(nx, ny, 0, nr)
            elapsed = time.time() - tstart
            print("%.2fs, %d%%, ETA %.2fs" % (elapsed, 100, 0.0))  # display.clj:20-24
            filtered = _denoise_frame(ds, nx, ny, lin, err, dn_iterations, dn_samples)
        finally:
            ds.ctx.progressive_release()
            ds.close()
    elif adaptive_denoised is not None:
        ds = DeviceScene(sc)
        try:
            na = FEATURE_SAMPLES if dn_samples is None else dn_samples
            for k, lin, rgb8, err, smp, cnt, active, flt, filtered, ferr in ds.refine_adaptive_denoised(nx, ny, nr, chunk, adaptive_denoised, na=na,
                                                                                                      iterations=dn_iterations):
                elapsed = _show_progress(tstart, k, nr)
                if budget is not None and elapsed > budget and k < nr and active:
                    print("stopped at %d of %d samples (budget %gs)" % (k, nr, budget))
                    break
            active, total, pixel_samples = ds.ctx.adaptive_status()
            print("samples: mean %.2f of %d per pixel, %d of %d tiles converged" % (pixel_samples / max(int(cnt[1]), 1), nr, total - active, total))
        finally:
            ds.ctx.progressive_release()
            ds.close()
    elif adaptive is not None:
        ds = DeviceScene(sc)
        try:
            for k, lin, rgb8, err, smp, cnt, active in ds.refine_adaptive(nx, ny, nr, chunk, adaptive):
                elapsed = _show_progress(tstart, k, nr)
                if budget is not None and elapsed > budget and k < nr and active:
                    print("stopped at %d of %d samples (budget %gs)" % (k, nr, budget))
                    break
            active, total, pixel_samples = ds.ctx.adaptive_status()
            print("samples: mean %.2f of %d per pixel, %d of %d tiles converged" % (pixel_samples / max(int(cnt[1]), 1), nr, total - active, total))
            if dn_iterations is not None:
                filtered = _denoise_frame(ds, nx, ny, lin, err, dn_iterations, dn_samples)
        finally:
            ds.ctx.progressive_release()
            ds.close()
    else:
        ds = DeviceScene(sc)
        try:
            for k, lin, rgb8, err, cnt in ds.refine(nx, ny, nr, chunk):
                elapsed = _show_progress(tstart, k, nr)
                why = None
                if budget is not None and elapsed > budget:
                    why = "budget %gs" % budget
                elif noise is not None and np.mean(err <= noise) >= 0.99:
                    why = "noise %g" % noise
                if why and k < nr:
                    print("stopped at %d of %d samples (%s)" % (k, nr, why))
                    break
            if dn_iterations is not None:
                filtered = _denoise_frame(ds, nx, ny, lin, err, dn_iterations, dn_samples)
        finally:
            ds.ctx.progressive_release()
            ds.close()
    print("total-rays %d total-pixels %d" % (int(cnt[0]), int(cnt[1])))  # metrics.clj:8-9
    _save_image(name, rgb8)
    if filtered is not None:
        _save_image(_denoised_name(name), filtered)
    if ao is not None:
        ds = DeviceScene(sc)
        try:
            vis = ds.ambient_occlusion_device(nx, ny, ao[0], ao[1]) if ao_on_device else ds.ambient_occlusion(nx, ny, ao[0], ao[1])
        finally:
            ds.close()
        grey = np.floor(255.0 * vis + 0.5).astype(np.uint8)
        _save_image(_ao_name(name), np.ascontiguousarray(np.repeat(grey[:, :, None], 3, axis=2)))
    if direct is not None:
        ds = DeviceScene(sc)
        try:
            lit = ds.render_direct(nx, ny, direct)[1]
        finally:
            ds.close()
        _save_image(_direct_name(name), lit)
    if nee:
        ds = DeviceScene(sc)
        try:
            lit = ds.render_nee(nx, ny, nr, min(nr, 16))[1]
        finally:
            ds.close()
        _save_image(_nee_name(name), lit)
    if mis is not None:
        ds = DeviceScene(sc)
        try:
            lit = ds.render_nee(nx, ny, nr, min(nr, 16), mis=True, light_choice=mis)[1]
        finally:
            ds.close()
        _save_image(_mis_name(name), lit)
    lit_eps = adaptive if adaptive is not None else adaptive_denoised  # the frame's stopping rule is the light-sampled frame's too
    for mode, volume, out_name in ((lit_mode, False, _lit_name(name)), (vol_mode, True, _lit_vol_name(name))):
        if mode is None:
            continue
        if devices is not None:  # one replica per listed device: the same frame, bit for bit
            from . import dist
            md = dist.MultiDevice(sc, devices)
            try:
                kw = dict(estimator=mode[0], volume=volume, light_choice=mode[1])
                if lit_eps is None:
                    frame = md.render_lit(nx, ny, nr, chunk=chunk, **kw)[1]
                else:
                    more = {} if adaptive is not None else dict(denoised=True, na=FEATURE_SAMPLES if dn_samples is None else dn_samples, iterations=dn_iterations)
                    frame, smp = md.refine_lit_adaptive(nx, ny, nr, chunk, lit_eps, **kw, **more)[1:4:2]
                    print("%s: %.1f%% of the %d pixel-samples taken" % ("--lit-vol" if volume else "--lit", 100.0 * float(smp.sum()) / (nx * ny * nr), nx * ny * nr))
            finally:
                md.close()
            _save_image(out_name, frame)
            continue
        ds = DeviceScene(sc)
        try:
            if lit_eps is None and mode[0] == "ris":
                frame = ds.render_lit_ris(nx, ny, nr, chunk=chunk)[1]
            elif lit_eps is None:
                frame = (ds.render_lit_vol if volume else ds.render_lit)(nx, ny, nr, chunk=chunk, estimator=mode[0], light_choice=mode[1])[1]
            else:
                more = {} if adaptive is not None else dict(denoised=True, na=FEATURE_SAMPLES if dn_samples is None else dn_samples, iterations=dn_iterations)
                frame, smp = ds.refine_lit_adaptive(nx, ny, nr, chunk, lit_eps, estimator=mode[0], volume=volume, light_choice=mode[1], **more)[1:4:2]
                print("%s: %.1f%% of the %d pixel-samples taken" % ("--lit-vol" if volume else "--lit", 100.0 * float(smp.sum()) / (nx * ny * nr), nx * ny * nr))
        finally:
            ds.close()
        _save_image(out_name, frame)
    return 0


if __name__ == "__main__":
    sys.exit(main())
