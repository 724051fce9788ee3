"""Host mirror of raytrace-clj.camera (src/raytrace_clj/camera.clj).

The constructors (camera.clj:18-33, 50-66) stay on the host, in the reference's operation order
(core.matrix ops restated with numpy float64: normalise = v * (1/|v|), cross, scalar*vector);
`get-ray` (camera.clj:8-16, 35-48) runs on the device."""
import math
from dataclasses import dataclass

import numpy as np


class Camera:
    """(defprotocol Camera (get-ray [this u v])) -- camera.clj:5-6"""

    def get_ray(self, u, v, key=0):
        from . import core
        return core.get_ray(self, u, v, key)


@dataclass(eq=False)
class PinholeCamera(Camera):  # camera.clj:8
    origin: np.ndarray
    lleft: np.ndarray
    horiz: np.ndarray
    vert: np.ndarray


@dataclass(eq=False)
class ThinLensCamera(Camera):  # camera.clj:35
    origin: np.ndarray
    lleft: np.ndarray
    horiz: np.ndarray
    vert: np.ndarray
    u: np.ndarray
    v: np.ndarray
    w: np.ndarray
    aperture: float
    t0: float
    t1: float


def _normalise(a):
    d = math.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    return a * (1.0 / d) if d > 0 else a.copy()


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], np.float64)


def _basis(lookfrom, lookat, vup, vfov, aspect):
    theta = float(vfov) * (math.pi / 180.0)
    half_height = math.tan(theta / 2.0)
    half_width = float(aspect) * half_height
    w = _normalise(lookfrom - lookat)
    u = _normalise(_cross(vup, w))
    v = _cross(w, u)
    return half_height, half_width, u, v, w


def pinhole_camera(*, lookfrom, lookat, vup, vfov, aspect):
    """(pinhole-camera :lookfrom :lookat :vup :vfov :aspect) -- camera.clj:18-33"""
    lookfrom, lookat, vup = (np.asarray(x, np.float64) for x in (lookfrom, lookat, vup))
    hh, hw, u, v, w = _basis(lookfrom, lookat, vup, vfov, aspect)
    return PinholeCamera(lookfrom, lookfrom - ((u * hw + v * hh) + w), u * (2.0 * hw), v * (2.0 * hh))


def thin_lens_camera(*, lookfrom, lookat, vup, vfov, aspect, aperture, focus_dist, t0, t1):
    """(thin-lens-camera ...) -- camera.clj:50-66"""
    lookfrom, lookat, vup = (np.asarray(x, np.float64) for x in (lookfrom, lookat, vup))
    hh, hw, u, v, w = _basis(lookfrom, lookat, vup, vfov, aspect)
    fd = float(focus_dist)
    lleft = lookfrom - ((u * (fd * hw) + v * (fd * hh)) + w * fd)
    return ThinLensCamera(lookfrom, lleft, u * ((2.0 * fd) * hw), v * ((2.0 * fd) * hh), u, v, w,
                          float(aperture), float(t0), float(t1))


# ---- moving the camera of a live scene (DeviceScene.set_camera): the reference has no such operation, a new view is a new record ----
_POINTS = ("origin", "lleft")
_VECTORS = ("horiz", "vert", "u", "v", "w")


def rotate_y(camera, angle, pivot):
    """The same record type turned rigidly by `angle` radians about the vertical axis through `pivot`: x' = c x + s z, z' = -s x + c z
    (RotateY's outward map, hitable.clj:441-443), the points (origin, lleft) about the pivot, the vectors (horiz, vert, u, v, w) about the
    origin; aperture and shutter are kept.  An angle whose sine is 0 and cosine 1 is the identity: the arrays are copied bit for bit."""
    s, c = math.sin(float(angle)), math.cos(float(angle))
    pivot = np.asarray(pivot, np.float64)
    identity = s == 0.0 and c == 1.0

    def turn(a, about):  # the height is copied, never computed
        x, z = a[0] - about[0], a[2] - about[2]
        return np.array([(c * x + s * z) + about[0], a[1], (-(s * x) + c * z) + about[2]], np.float64)

    fields = {}
    for name in _POINTS + _VECTORS:
        if not hasattr(camera, name):
            continue
        a = np.asarray(getattr(camera, name), np.float64)
        fields[name] = a.copy() if identity else turn(a, pivot if name in _POINTS else np.zeros(3))
    if isinstance(camera, ThinLensCamera):
        return ThinLensCamera(aperture=camera.aperture, t0=camera.t0, t1=camera.t1, **fields)
    if isinstance(camera, PinholeCamera):
        return PinholeCamera(**fields)
    raise TypeError("rotate_y: %s is not a camera record" % type(camera).__name__)


def view_pivot(camera):
    """A point on the camera's look-at axis, from the record alone: the centre of its image plane, lleft + horiz / 2 + vert / 2 (the
    focus point origin - focus-dist * w of a thin lens: the look-at point itself when the lens is focused on it)."""
    return np.asarray(camera.lleft, np.float64) + 0.5 * np.asarray(camera.horiz, np.float64) + 0.5 * np.asarray(camera.vert, np.float64)


def orbit(camera, n, pivot=None):
    """n views of a turntable: view k is `camera` turned by k * 360 / n degrees about the vertical axis through `pivot` (default: view_pivot)"""
    pivot = view_pivot(camera) if pivot is None else np.asarray(pivot, np.float64)
    return [rotate_y(camera, 2.0 * math.pi * k / n, pivot) for k in range(n)]


# ---- ray generators for DeviceScene.render_rays / render_with: camera models the device does not have, as rays ----
# A generator returns (rays [nx * ny * s_count, 7] float64, ctr0) for samples [s_first, s_first + s_count) of an nx x ny image, grouped per pixel:
# group g = j * nx + i in the reference's coordinates (j = 0 is the bottom row), ray r of the group is sample s_first + r.  Its jitter is draws 0
# and 1 of the stream keyed sample_key(seed, j * nx + i, s) -- the key render_rays derives for that row when it is given none -- so ctr0 = 2: the
# path continues the stream where the generator stopped, as a camera path does.
def _pixel_samples(nx, ny, s_first, s_count, seed):
    from . import util
    if nx <= 0 or ny <= 0 or s_first < 0 or s_count <= 0:
        raise ValueError("nx, ny, s_count must be > 0 and s_first >= 0")
    pix, ss = (a.ravel() for a in np.meshgrid(np.arange(nx * ny), np.arange(s_first, s_first + s_count), indexing="ij"))
    keys = util.sample_keys(seed, pix, ss)
    u = ((pix % nx).astype(np.float64) + util.draw_uniforms(keys, 0)) / np.float64(nx)
    v = ((pix // nx).astype(np.float64) + util.draw_uniforms(keys, 1)) / np.float64(ny)
    return u, v


def _rays(origin, direction, time):
    n = len(direction)
    rays = np.empty((n, 7), np.float64)
    rays[:, 0:3] = origin
    rays[:, 3:6] = direction
    rays[:, 6] = time
    return rays, 2


def panorama_rays(nx, ny, s_first, s_count, *, lookfrom, lookat, vup, seed=0x5EED0002, time=0.0):
    """Equirectangular panorama: the full sphere seen from `lookfrom`.  Longitude (u - 1/2) * 2 pi about the axis `vup`, latitude (v - 1/2) * pi:
    the top row (j = ny - 1) closes on +vup, the bottom row on -vup, and the centre column is the meridian through lookat - lookfrom (the centre
    pixel looks along it when vup is perpendicular to it).  Directions are unit vectors up to rounding.  Time: no draw is made, as the pinhole
    camera makes none; every ray carries `time` (default 0.0, the pinhole camera's)."""
    lookfrom, lookat, vup = (np.asarray(x, np.float64) for x in (lookfrom, lookat, vup))
    up = _normalise(vup)
    d = lookat - lookfrom
    fwd = _normalise(d - up * ((d[0] * up[0] + d[1] * up[1]) + d[2] * up[2]))
    right = _cross(fwd, up)
    u, v = _pixel_samples(nx, ny, s_first, s_count, seed)
    lon, lat = (u - 0.5) * (2.0 * math.pi), (v - 0.5) * math.pi
    cl = np.cos(lat)
    direction = (cl * np.cos(lon))[:, None] * fwd + (cl * np.sin(lon))[:, None] * right + np.sin(lat)[:, None] * up
    return _rays(lookfrom, direction, float(time))


def orthographic_rays(nx, ny, s_first, s_count, *, lookfrom, lookat, vup, width, seed=0x5EED0002, time=0.0):
    """Orthographic view: parallel rays along lookat - lookfrom (a unit vector) from a window of `width` x `width * ny / nx` centred on `lookfrom`
    in the plane through it perpendicular to that direction; the window's axes are the pinhole camera's u and v (camera.clj:18-33).  Time: no
    draw is made; every ray carries `time` (default 0.0, the pinhole camera's)."""
    lookfrom, lookat, vup = (np.asarray(x, np.float64) for x in (lookfrom, lookat, vup))
    w = _normalise(lookfrom - lookat)
    cu = _normalise(_cross(vup, w))
    cv = _cross(w, cu)
    height = float(width) * ny / nx
    u, v = _pixel_samples(nx, ny, s_first, s_count, seed)
    origin = lookfrom + ((u - 0.5) * float(width))[:, None] * cu + ((v - 0.5) * height)[:, None] * cv
    return _rays(origin, np.broadcast_to(-w, (len(u), 3)), float(time))


# ---- secondary rays for DeviceScene.occluded / ambient_occlusion: not a camera, a hemisphere over every surface point ----
def hemisphere_rays(points, normals, n_dirs, first=0, seed=0x5EED0002, time=0.0):
    """n_dirs rays from each of `points` [n, 3] into the hemisphere about `normals` [n, 3] (any length > 0; the rays leave on the normal's side),
    cosine-weighted by Malley's method: a uniform point of the unit disk (radius sqrt(xi0), angle 2 pi xi1) lifted onto the hemisphere, in an
    orthonormal frame about the normal.  Ray r of point g is row g * n_dirs + r and takes draws 0 and 1 of the stream keyed
    sample_key(seed, g, first + r): numpy only, so any split of a point's directions over `first` gives the rays of one call.  Directions are unit
    vectors up to rounding with normal . direction = sqrt(1 - xi0) > 0.  -> rays [n * n_dirs, 7] float64, every ray carrying `time`."""
    from . import util
    points, normals = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(normals, np.float64).reshape(-1, 3)
    n_dirs, first = int(n_dirs), int(first)
    if len(points) != len(normals) or n_dirs <= 0 or first < 0:
        raise ValueError("points and normals must pair up, n_dirs > 0 and first >= 0")
    g, r = (a.ravel() for a in np.meshgrid(np.arange(len(points)), np.arange(first, first + n_dirs), indexing="ij"))
    keys = util.sample_keys(seed, g, r)
    xi0, xi1 = util.draw_uniforms(keys, 0), util.draw_uniforms(keys, 1)
    rad, phi = np.sqrt(xi0), (2.0 * math.pi) * xi1
    x, y, z = rad * np.cos(phi), rad * np.sin(phi), np.sqrt(1.0 - xi0)
    with np.errstate(invalid="ignore", divide="ignore"):
        n = normals / np.sqrt((normals * normals).sum(axis=1))[:, None]
        # the frame: the coordinate axis least aligned with the normal, made perpendicular to it
        axis = np.where((np.abs(n[:, 0]) < 0.5)[:, None], np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
        t = np.cross(axis, n)
        t = t / np.sqrt((t * t).sum(axis=1))[:, None]
    b = np.cross(n, t)
    direction = x[:, None] * t[g] + y[:, None] * b[g] + z[:, None] * n[g]
    return _rays(points[g], direction, float(time))[0]


def hemisphere_rays_disk(points, normals, n_dirs, first=0, seed=0x5EED0002, time=0.0):
    """hemisphere_rays with the sampler the device runs (include/rtmi.h, "the hemisphere rule", steps 3 - 7): the same signature and row order, the
    same cosine weighting by Malley's method, but the uniform point of the unit disk comes from the reference's rand-in-unit-disk rejection loop
    (util.clj:32-41) instead of a radius and an angle -- no cos, no sin, only + - * / sqrt, every one a single IEEE operation in the header's
    order, so rtmi_occlusion_hemisphere's out_rays equal these rows bit for bit.  Ray r of point g takes candidates (draws 2c, 2c + 1 as 2 u - 1)
    of the stream keyed sample_key(seed, g, first + r) until one lies inside the disk.  -> rays [n * n_dirs, 7] float64, every ray carrying `time`."""
    from . import util
    points, normals = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(normals, np.float64).reshape(-1, 3)
    n_dirs, first = int(n_dirs), int(first)
    if len(points) != len(normals) or n_dirs <= 0 or first < 0:
        raise ValueError("points and normals must pair up, n_dirs > 0 and first >= 0")
    g, r = (a.ravel() for a in np.meshgrid(np.arange(len(points)), np.arange(first, first + n_dirs), indexing="ij"))
    keys = util.sample_keys(seed, g, r)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nx, ny, nz = normals[:, 0], normals[:, 1], normals[:, 2]
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)                               # 3. nn = n / sqrt(dot3(n, n))
        nx, ny, nz = nx / length, ny / length, nz / length
        small = np.abs(nx) < 0.5                                                        # 4. the tangent
        zero = np.zeros(len(nx))
        tx, ty, tz = np.where(small, zero, nz), np.where(small, -nz, zero), np.where(small, ny, -nx)
        tl = np.sqrt((tx * tx + ty * ty) + tz * tz)
        tx, ty, tz = tx / tl, ty / tl, tz / tl
        bx, by, bz = ny * tz - nz * ty, nz * tx - nx * tz, nx * ty - ny * tx            # 5. b = nn x t
        x, y = np.zeros(len(keys)), np.zeros(len(keys))                                 # 6. the first candidate inside the disk
        pending, c = np.arange(len(keys)), 0
        while len(pending):
            cx = 2.0 * util.draw_uniforms(keys[pending], 2 * c) - 1.0
            cy = 2.0 * util.draw_uniforms(keys[pending], 2 * c + 1) - 1.0
            inside = ~(((cx * cx + cy * cy) + 0.0 * 0.0) >= 1.0)
            x[pending[inside]], y[pending[inside]] = cx[inside], cy[inside]
            pending, c = pending[~inside], c + 1
        z = np.sqrt(1.0 - (x * x + y * y))                                              # 7. lifted onto the hemisphere
        dx = (x * tx[g] + y * bx[g]) + z * nx[g]
        dy = (x * ty[g] + y * by[g]) + z * ny[g]
        dz = (x * tz[g] + y * bz[g]) + z * nz[g]
    return _rays(points[g], np.stack([dx, dy, dz], axis=1), float(time))[0]


LIGHT_REC = 10  # doubles per light of a light table: kind, 5 geometry doubles, area, Le rgb
FOURPI = float.fromhex("0x1.921fb54442d18p+3")


def light_table(flat, prims):
    """The light table rtmi_direct_irradiance builds for the primitives `prims` of a FlatScene (each out of DeviceScene.lights()) -> [n, LIGHT_REC]:
    the primitive's kind; a sphere's centre and radius and 0, or a rectangle's a0, b0, a1, b1, k; the area FOURPI * (r * r) or
    |(a1 - a0) * (b1 - b0)|; Le = the colour of the DiffuseLight's Constant texture."""
    prims = np.asarray(prims, np.int64).reshape(-1)
    kind = np.asarray(flat.prim_kind, np.int64)[prims]
    geom = np.asarray(flat.prim_geom, np.float64).reshape(-1, 9)[prims]
    tex = np.asarray(flat.mat_tex, np.int64)[np.asarray(flat.prim_mat, np.int64)[prims]]
    sphere = kind <= 1
    table = np.zeros((len(prims), LIGHT_REC), np.float64)
    table[:, 0] = kind
    table[:, 1:5] = geom[:, 0:4]
    table[:, 5] = np.where(sphere, 0.0, geom[:, 4])
    table[:, 6] = np.where(sphere, FOURPI * (geom[:, 3] * geom[:, 3]), np.abs((geom[:, 2] - geom[:, 0]) * (geom[:, 3] - geom[:, 1])))
    table[:, 7:10] = np.asarray(flat.tex_param, np.float64).reshape(-1, 12)[tex, 0:3]
    return table


def _light_terms(px, py, pz, nx, ny, nz, rows, keys, lobe=True):
    """Steps 3 - 5 of the light rule for one item per entry: the point p, the UNIT normal (nx, ny, nz), the item's light record `rows` [items, LIGHT_REC]
    and its stream `keys` -> (dx, dy, dz, d2, cp, cl, built, area), every operation a single IEEE operation in the header's order.  lobe=False (a
    vertex inside a medium: no normal, vol_samples): cp > 0 is not asked for."""
    from . import util
    kind = rows[:, 0].astype(np.int64)
    sphere = kind <= 1
    g0, g1, g2, g3, g4, area = (rows[:, c] for c in range(1, 7))
    a = g0 + util.draw_uniforms(keys, 0) * (g2 - g0)                                    # 3. a rectangle: draws 0 and 1
    b = g1 + util.draw_uniforms(keys, 1) * (g3 - g1)
    x, y = np.zeros(len(keys)), np.zeros(len(keys))                                     # 4. a sphere: the first candidate inside the disk
    pending, c = np.flatnonzero(sphere), 0
    while len(pending):
        cx = 2.0 * util.draw_uniforms(keys[pending], 2 * c) - 1.0
        cy = 2.0 * util.draw_uniforms(keys[pending], 2 * c + 1) - 1.0
        inside = ~(((cx * cx + cy * cy) + 0.0 * 0.0) >= 1.0)
        x[pending[inside]], y[pending[inside]] = cx[inside], cy[inside]
        pending, c = pending[~inside], c + 1
    S = x * x + y * y
    root = np.sqrt(1.0 - S)
    sx = np.where(sphere, (2.0 * x) * root, np.where(kind == 5, 1.0, 0.0))
    sy = np.where(sphere, (2.0 * y) * root, np.where(kind == 4, 1.0, 0.0))
    sz = np.where(sphere, 1.0 - 2.0 * S, np.where(kind == 3, 1.0, 0.0))
    qx = np.where(sphere, g0 + g3 * sx, np.where(kind == 5, g4, a))
    qy = np.where(sphere, g1 + g3 * sy, np.where(kind == 3, b, np.where(kind == 4, g4, a)))
    qz = np.where(sphere, g2 + g3 * sz, np.where(kind == 3, g4, b))
    dx, dy, dz = qx - px, qy - py, qz - pz                                              # 5. the geometry term
    d2 = (dx * dx + dy * dy) + dz * dz
    cp = (nx * dx + ny * dy) + nz * dz
    sd = (sx * dx + sy * dy) + sz * dz
    cl = np.abs(sd)
    ex, ey, ez = px - g0, py - g1, pz - g2
    far = sphere & (((ex * ex + ey * ey) + ez * ez) > g3 * g3) & (sd > 0.0)               # the far side of a sphere seen from outside
    built = ~far & (d2 > 0.0) & ((cp > 0.0) if lobe else True) & (cl > 0.0)
    return dx, dy, dz, d2, cp, cl, built, area


def light_samples(points, normals, lights, n_samples, first=0, seed=0x5EED0002, time=0.0):
    """The shadow rays and weights the device builds towards area lights (include/rtmi.h, "the light rule", steps 2 - 6), every operation a single
    IEEE operation in the header's order, so rtmi_direct_irradiance's out_rays equal these rows bit for bit.  points, normals [n, 3]: the shaded
    points and their normals on the viewer's side (any length; the rule normalises them); lights [n_lights, LIGHT_REC] (light_table).  Item
    (g * n_samples + k) * n_lights + l is sample first + k of point g on light l, its stream keyed sample_key(seed, g * n_lights + l, first + k):
    a rectangle takes draws 0 and 1 as in-plane coordinates, a sphere the rejection loop's disk point mapped onto the sphere by Marsaglia's method.
    -> (rays [items, 7] from the point to the sampled point, so t = 1 is the light; weights [items] = cos cos' area / d^2 as
    ((cp * cl) / (d2 * d2)) * area; built [items] bool: False where the light is behind the point, edge-on, or turns its far side -- those rows
    are zeros).  The irradiance estimate of a point is the mean over k of the sum over l of Le * weight * visibility."""
    from . import util
    points, normals = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(normals, np.float64).reshape(-1, 3)
    lights = np.asarray(lights, np.float64).reshape(-1, LIGHT_REC)
    n_samples, first, nl = int(n_samples), int(first), len(lights)
    if len(points) != len(normals) or n_samples <= 0 or first < 0:
        raise ValueError("points and normals must pair up, n_samples > 0 and first >= 0")
    g, k, l = (a.ravel() for a in np.meshgrid(np.arange(len(points)), np.arange(first, first + n_samples), np.arange(nl), indexing="ij"))
    keys = util.sample_keys(seed, g * nl + l, k)                                        # 2. the item's stream
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nx, ny, nz = normals[:, 0], normals[:, 1], normals[:, 2]
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)                               # (step 3 of the hemisphere rule)
        nx, ny, nz = (nx / length)[g], (ny / length)[g], (nz / length)[g]
        dx, dy, dz, d2, cp, cl, built, area = _light_terms(points[g, 0], points[g, 1], points[g, 2], nx, ny, nz, lights[l], keys)
        w = ((cp * cl) / (d2 * d2)) * area
    rays = _rays(points[g], np.stack([dx, dy, dz], axis=1), float(time))[0]            # 6. origin p, direction d: t = 1 is the light
    rays[~built] = 0.0
    return rays, np.where(built, w, 0.0), built


TWO_INV_PI = float.fromhex("0x1.45f306dc9c883p-1")


def nee_samples(points, normals, lights, keys_sample, keys_pick, light=None):
    """The light samples of light-sampled paths (include/rtmi.h, "the NEE rule", steps 2 - 4), one per vertex, every operation a single IEEE
    operation in the header's order, so rtmi_probe_paths_nee's log columns [13..17] equal these bit for bit.  points, normals [n, 3]: the hit
    points and the records' normals AS THEY ARE (no viewer-side flip; the rule normalises them); lights [nl, LIGHT_REC] (light_table), nl >= 1;
    keys_sample, keys_pick [n] uint64: sample_key(K, j, 0) and sample_key(K, j, 1) of the path keyed K at its vertex j.  The light is
    min(int(u * nl), nl - 1) with u = draw 0 of keys_pick (or `light` [n], where given); the point on it comes from keys_sample as in light_samples.
    -> (light [n] int, d [n, 3] = sampled point - p (zeros where no ray is built), w [n] = the reference's lobe 2 cos^3 / pi times the light's
    cosine, its area and the inverse square, as ((((cp*cp)*(cp*cl)) / ((d2*d2)*d2)) * area) * TWO_INV_PI (0 where no ray is built), built [n])."""
    from . import util
    points, normals = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(normals, np.float64).reshape(-1, 3)
    lights = np.asarray(lights, np.float64).reshape(-1, LIGHT_REC)
    keys_sample, keys_pick = np.asarray(keys_sample, np.uint64).reshape(-1), np.asarray(keys_pick, np.uint64).reshape(-1)
    nl = len(lights)
    if not (len(points) == len(normals) == len(keys_sample) == len(keys_pick)) or nl < 1:
        raise ValueError("points, normals and keys must pair up, and there must be a light")
    l = np.minimum((util.draw_uniforms(keys_pick, 0) * np.float64(nl)).astype(np.int64), nl - 1)   # 2. which light
    if light is not None:                                                               # (the MIS rule's pick, mis_pick, in its place)
        l = np.asarray(light, np.int64).reshape(-1)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        nx, ny, nz = normals[:, 0], normals[:, 1], normals[:, 2]
        len2 = (nx * nx + ny * ny) + nz * nz
        sound = np.isfinite(points).all(axis=1) & np.isfinite(normals).all(axis=1) & (len2 > 0.0)
        length = np.sqrt(len2)                                                          # (step 3 of the hemisphere rule; no flip)
        dx, dy, dz, d2, cp, cl, built, area = _light_terms(points[:, 0], points[:, 1], points[:, 2], nx / length, ny / length, nz / length,
                                                           lights[l], keys_sample)
        built = built & sound
        w = ((((cp * cp) * (cp * cl)) / ((d2 * d2) * d2)) * area) * TWO_INV_PI        # 4. the weight
    d = np.stack([dx, dy, dz], axis=1)
    d[~built] = 0.0
    return l, d, np.where(built, w, 0.0), built


def mis_pick(lights, keys_pick, light_choice=0):
    """Step 2 of the MIS rule (include/rtmi.h): which light each vertex samples, and the inverse pick probability q of every light.
    light_choice 0: the NEE rule's uniform pick, q = nl.  light_choice 1, by power: omega_l = area_l * ((Le.r + Le.g) + Le.b), C = the running sum in
    list order, W = C[nl - 1]; the light is the first index with u * W < C_l (else nl - 1) for the same draw u, and q_l = W / omega_l; if W is not finite
    and > 0 the pick is the uniform one.  -> (light [n] int, q [nl], live [nl] bool: False for a light by power with omega = 0, which is never picked
    and whose closing emission is kept whole)."""
    from . import util
    lights = np.asarray(lights, np.float64).reshape(-1, LIGHT_REC)
    keys_pick = np.asarray(keys_pick, np.uint64).reshape(-1)
    nl = len(lights)
    if nl < 1 or light_choice not in (0, 1):
        raise ValueError("there must be a light, and light_choice is 0 (uniform) or 1 (by power)")
    u = util.draw_uniforms(keys_pick, 0)
    uniform = (np.minimum((u * np.float64(nl)).astype(np.int64), nl - 1), np.full(nl, np.float64(nl)), np.ones(nl, bool))
    if light_choice == 0:
        return uniform
    with np.errstate(all="ignore"):
        omega = lights[:, 6] * ((lights[:, 7] + lights[:, 8]) + lights[:, 9])
        C = omega.copy()
        for k in range(1, nl):
            C[k] = C[k - 1] + omega[k]
        W = C[nl - 1]
        if not (np.isfinite(W) and W > 0.0):
            return uniform
        below = (u * W)[:, None] < C[None, :]
        light = np.where(below.any(axis=1), below.argmax(axis=1), nl - 1)
        return light, W / omega, omega != 0.0


def mis_weight(w, q):
    """Step 4 of the MIS rule: x = w * q, the ratio p_scatter / p_light of the two strategies' densities at the sampled point, and the balance
    heuristic's share of the light sample m = x / (1 + x), 1 where x is +inf -> (x, m).  T * Le * m is bounded by T * Le whatever w is."""
    w, q = np.asarray(w, np.float64), np.asarray(q, np.float64)
    with np.errstate(all="ignore"):
        x = w * q
        m = np.where(x == np.inf, 1.0, x / (1.0 + x))
    return x, m


def mis_lobe(normals, dirs, points=None):
    """Step 6 of the MIS rule: g = ((a*a)*a) / ((DD*DD)*DD) with a = dot3(nn, D), DD = dot3(D, D), nn the normalised normal and D the scattered
    direction (any length) -- the reference's lobe 2 cos^3 / pi less its constant; +0.0 where the normal (or the point, if given) is not finite, the
    normal has no length, or a > 0 and DD > 0 do not both hold."""
    normals, dirs = np.asarray(normals, np.float64).reshape(-1, 3), np.asarray(dirs, np.float64).reshape(-1, 3)
    with np.errstate(all="ignore"):
        nx, ny, nz = normals[:, 0], normals[:, 1], normals[:, 2]
        len2 = (nx * nx + ny * ny) + nz * nz
        valid = np.isfinite(normals).all(axis=1) & (len2 > 0.0)
        if points is not None:
            valid &= np.isfinite(np.asarray(points, np.float64).reshape(-1, 3)).all(axis=1)
        length = np.sqrt(len2)
        nx, ny, nz = nx / length, ny / length, nz / length
        Dx, Dy, Dz = dirs[:, 0], dirs[:, 1], dirs[:, 2]
        a = (nx * Dx + ny * Dy) + nz * Dz
        DD = (Dx * Dx + Dy * Dy) + Dz * Dz
        g = ((a * a) * a) / ((DD * DD) * DD)
    return np.where(valid & (a > 0.0) & (DD > 0.0), g, 0.0)


def mis_closing(g, normals, dirs, t, area, q):
    """Step 7 of the MIS rule where the closing emission is weighted: the emitter record's normal normalised to s', cl' = |dot3(s', D)| for the arriving
    direction D, x' = ((((g * cl') / (t*t)) * area) * TWO_INV_PI) * q and m' = x' / (1 + x'), 1 where x' is +inf, +0.0 where it is NaN -> (x', m')."""
    normals, dirs = np.asarray(normals, np.float64).reshape(-1, 3), np.asarray(dirs, np.float64).reshape(-1, 3)
    g, t, area, q = (np.asarray(a, np.float64) for a in (g, t, area, q))
    with np.errstate(all="ignore"):
        nx, ny, nz = normals[:, 0], normals[:, 1], normals[:, 2]
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        nx, ny, nz = nx / length, ny / length, nz / length
        cl = np.abs((nx * dirs[:, 0] + ny * dirs[:, 1]) + nz * dirs[:, 2])
        x = ((((g * cl) / (t * t)) * area) * TWO_INV_PI) * q
        m = np.where(np.isnan(x), 0.0, np.where(x == np.inf, 1.0, x / (1.0 + x)))
    return x, m


def ris_candidates(points, normals, lights, path_keys, segments):
    """Step 2 of the proposal rule (include/rtmi.h): every light of lights [nl, LIGHT_REC] proposes one point at every vertex -- nee_samples with the
    stream keyed sample_key(K, j, 4 * l) for light l, K = path_keys [n] and j = segments [n] -- and is weighed: x = w (q = 1: mis_weight),
    m = x / (1 + x), lum = (Le.r + Le.g) + Le.b, what = lum * m; a candidate is live if it built a ray and 0 < what < +inf (a NaN fails).
    -> (d [n, nl, 3], w [n, nl], m [n, nl], what [n, nl], live [n, nl] bool, lum [nl])."""
    from . import util
    points, normals = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(normals, np.float64).reshape(-1, 3)
    lights = np.asarray(lights, np.float64).reshape(-1, LIGHT_REC)
    path_keys, segments = np.asarray(path_keys, np.uint64).reshape(-1), np.asarray(segments, np.uint64).reshape(-1)
    n, nl = len(points), len(lights)
    lum = (lights[:, 7] + lights[:, 8]) + lights[:, 9]
    d, w, m, what, live = np.zeros((n, nl, 3)), np.zeros((n, nl)), np.zeros((n, nl)), np.zeros((n, nl)), np.zeros((n, nl), bool)
    for l in range(nl):
        keys = util.sample_keys(path_keys, segments, np.full(n, 4 * l, np.uint64))
        _, d[:, l], w[:, l], built = nee_samples(points, normals, lights, keys, keys, light=np.full(n, l, np.int64))
        _, m[:, l] = mis_weight(w[:, l], 1.0)
        with np.errstate(all="ignore"):
            what[:, l] = lum[l] * m[:, l]
        live[:, l] = built & (what[:, l] > 0.0) & (what[:, l] < np.inf)
    return d, w, m, what, live, lum


def ris_choose(what, live, path_keys, segments):
    """Step 3 of the proposal rule: the one-pass weighted reservoir over the candidates of ris_candidates, in list order.  S starts at +0.0 and grows
    by what_l at every live candidate; the first live candidate is taken, a later one replaces it if u_l * S < what_l, u_l = draw l of the stream keyed
    sample_key(K, j, 1).  -> (chosen [n] int (0 where none is live), S [n], what of the chosen [n] (0 where none), r = S / what (0 where none),
    live count [n] int)."""
    from . import util
    what, live = np.asarray(what, np.float64), np.asarray(live, bool)
    path_keys, segments = np.asarray(path_keys, np.uint64).reshape(-1), np.asarray(segments, np.uint64).reshape(-1)
    n, nl = what.shape
    kc = util.sample_keys(path_keys, segments, np.full(n, 1, np.uint64))
    S, sel, sel_what, count = np.zeros(n), np.zeros(n, np.int64), np.zeros(n), np.zeros(n, np.int64)
    for l in range(nl):
        with np.errstate(all="ignore"):
            S = np.where(live[:, l], S + what[:, l], S)
            take = live[:, l] & ((count == 0) | (util.draw_uniforms(kc, l) * S < what[:, l]))
        sel = np.where(take, l, sel)
        sel_what = np.where(take, what[:, l], sel_what)
        count = count + live[:, l]
    with np.errstate(all="ignore"):
        r = np.where(count > 0, S / sel_what, 0.0)
    return sel, S, sel_what, r, count


INV_4PI = float.fromhex("0x1.45f306dc9c883p-4")


def vol_samples(points, normals, iso, lights, keys_sample, keys_pick, light=None):
    """The light samples of light-sampled paths through participating media (include/rtmi.h, "the volume rule", steps 2 and 3), one per vertex,
    so rtmi_probe_paths_vol's log columns [13..17] equal these bit for bit.  iso [n] bool: the vertex is an Isotropic scatter inside a medium.
    A Lambertian vertex (iso False) is nee_samples' row.  At an Isotropic vertex the normal is not read: the vertex is valid when p is finite, a ray
    is built when d2 > 0, cl > 0 and the far-side rule allows it, and the weight carries the uniform sphere's density 1 / 4 pi in the lobe's place:
    w = ((cl / (d2 * sqrt(d2))) * area) * INV_4PI.  The pick and the point on the light are nee_samples' (`light`: the MIS rule's pick).
    -> nee_samples' tuple (light [n], d [n, 3], w [n], built [n])."""
    points, normals = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(normals, np.float64).reshape(-1, 3)
    iso = np.asarray(iso, bool).reshape(-1)
    if len(iso) != len(points):
        raise ValueError("iso must pair up with the points")
    lights = np.asarray(lights, np.float64).reshape(-1, LIGHT_REC)
    keys_sample = np.asarray(keys_sample, np.uint64).reshape(-1)
    unit = np.where(iso[:, None], np.array([0.0, 0.0, 1.0]), normals)                   # (an Isotropic row's normal is not read: its row is replaced below)
    l, d, w, built = nee_samples(points, unit, lights, keys_sample, keys_pick, light)
    k = np.flatnonzero(iso)
    if len(k):
        zero = np.zeros(len(k))
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            dx, dy, dz, d2, _, cl, bi, area = _light_terms(points[k, 0], points[k, 1], points[k, 2], zero, zero, zero, lights[l[k]], keys_sample[k],
                                                           lobe=False)
            bi = bi & np.isfinite(points[k]).all(axis=1)
            wi = ((cl / (d2 * np.sqrt(d2))) * area) * INV_4PI                           # 3. the weight at an Isotropic vertex
        d[k] = np.where(bi[:, None], np.stack([dx, dy, dz], axis=1), 0.0)
        w[k] = np.where(bi, wi, 0.0)
        built[k] = bi
    return l, d, w, built


def vol_lobe(normals, dirs, iso, points=None):
    """Step 5 of the volume rule: the MIS lobe value per vertex -- mis_lobe's at a Lambertian vertex; at an Isotropic one (iso True)
    g = 0.125 / (DD * sqrt(DD)) with DD = dot3(D, D) if the point (where given) is finite and DD > 0, else +0.0.  g * cl' / t^2 * area * TWO_INV_PI
    is then the weight of vol_samples at d = t * D (0.125 = INV_4PI / TWO_INV_PI, exact), which mis_closing forms."""
    dirs = np.asarray(dirs, np.float64).reshape(-1, 3)
    iso = np.asarray(iso, bool).reshape(-1)
    g = mis_lobe(normals, dirs, points)
    with np.errstate(all="ignore"):
        DD = (dirs[:, 0] * dirs[:, 0] + dirs[:, 1] * dirs[:, 1]) + dirs[:, 2] * dirs[:, 2]
        gi = 0.125 / (DD * np.sqrt(DD))
    valid = DD > 0.0
    if points is not None:
        valid = valid & np.isfinite(np.asarray(points, np.float64).reshape(-1, 3)).all(axis=1)
    return np.where(iso, np.where(valid, gi, 0.0), g)
