"""Scene and ray recipes for the tests of deep, degenerate and threshold-sized trees (test_tree_host.py on the CPU, test_gpu_deep_trees.py on
the device).  Host records and numpy only: nothing here touches a device.

Every recipe returns a list of Hitable records (the world's items, in Hitlist order); `scene(items, lens)` puts a camera in front of them.  The
camera of every recipe stands at CAMERA_AT: the builder's "big primitive" rule compares a primitive with the scene's bound, which includes the
camera's position, so the trees the host hook builds (rtmi_test_build_tree takes the camera's origin) are the trees the device scenes get.

HOST_TABLE holds, per recipe, what the builder reports for it: (node records, depth, grid cells per side, big primitives).  The depths of the
chains are the builder's answer to spheres whose sizes fall geometrically: the SAH keeps cutting the big end off (one level per cut) until the
depth budget forces median splits."""
import numpy as np

CAMERA_AT = (9.0, 0.5, 1.0)
STACK = 32  # RTMI_BVH_STACK (rtmi_device.h)

# recipe -> (node records, depth, grid cells per side, big primitives) as rtmi_test_build_tree / DeviceScene.tree_info report them
HOST_TABLE = {
    "chain(1000, 0.9, 0.15)": (999, 29, 0, 1),
    "chain(1000, 0.9, 0.9)": (999, 29, 0, 1),
    "chain(763, 0.95, 0.15)": (762, 27, 0, 1),
    "chain(400, 0.9, 0.15)": (399, 26, 0, 1),
    "chain(120, 0.9, 0.15)": (119, 14, 0, 1),
    "chain(60, 0.9, 0.15)": (59, 10, 0, 1),
    "chain(30, 0.9, 0.15)": (29, 7, 0, 1),
    "chain(60, 0.5, 0.15, dome=False)": (59, 22, 0, 0),
    "chain(200, 0.5, 0.15, dome=False)": (199, 27, 0, 0),
    "identical(300)": (299, 9, 0, 1),
    "identical(300, 12)": (311, 11, 0, 1),
    "shells(300)": (299, 9, 0, 1),
    "many_big(20, 300)": (303, 11, 0, 16),   # 300 small spheres + the four shells the cap of 16 sends into the tree
    "negative_radius(200)": (199, 10, 0, 1),
    "zero_radius(200)": (211, 10, 0, 1),
    "cloud(128)": (127, 9, 0, 1),            # 127 inner nodes: below the time-slicing threshold of 128
    "cloud(129)": (128, 9, 0, 1),
    "layer(255)": (254, 10, 0, 1),           # no entry grid below 256 layer primitives
    "layer(256)": (2399, 10, 9, 1),          # 9 x 9 cells, 4 x 81 rectangle trees behind the whole tree's 255 nodes
}


def build(name):
    """the items of a HOST_TABLE key"""
    return eval(name, {"__builtins__": {}}, {k: globals()[k] for k in ("chain", "identical", "shells", "many_big", "negative_radius", "zero_radius", "cloud", "layer")})


def _mods():
    import raytrace_clj_amd as r
    return r.hitable, r.shader, r.texture, r.camera


def _colour(k):
    return np.array([0.25 + 0.5 * ((k * 7) % 5) / 4.0, 0.25 + 0.5 * ((k * 3) % 7) / 6.0, 0.25 + 0.5 * ((k * 5) % 3) / 2.0])


def _materials():
    """three shared materials a recipe deals round robin (neighbours in the Hitlist differ, so a wrong winner shows in a frame), and the light"""
    H, S, T, _ = _mods()
    return ([S.lambertian(albedo=T.constant(color=_colour(1))), S.metal(albedo=T.constant(color=_colour(2)), fuzz=0.2), S.dielectric(ri=1.5)],
            S.diffuse_light(tex=T.constant(color=np.array([1.5, 1.5, 1.5]))))


def _dome(light, radius=60.0):
    H = _mods()[0]
    return H.sphere(center=np.zeros(3), radius=radius, material=light)


CHAIN_CAMERA_AT = (-2e-4, 1e-6, 2e-6)  # just beyond the small end of a chain, looking along it


def scene(items, lens=False, bvh=False, lookfrom=CAMERA_AT, lookat=(1.5, 0.0, 0.0), vfov=30.0, aperture=0.2, focus_dist=8.0):
    """{"camera", "world"}: a pinhole camera (one origin for all rays: 11 stash words) or a thin lens with a real aperture (17)"""
    H, _, _, C = _mods()
    at, to, up = np.array(lookfrom, np.float64), np.array(lookat, np.float64), np.array([0.0, 1.0, 0.0])
    if lens:
        camera = C.thin_lens_camera(lookfrom=at, lookat=to, vup=up, vfov=vfov, aspect=1.5, aperture=aperture, focus_dist=focus_dist, t0=0.0, t1=1.0)
    else:
        camera = C.pinhole_camera(lookfrom=at, lookat=to, vup=up, vfov=vfov, aspect=1.5)
    return {"camera": camera, "world": H.make_bvh(list(items), 0.0, 1.0) if bvh else H.hitlist(items=list(items))}


def chain_scene(items, lens=False):
    """a chain seen from just beyond its small end, 6 degrees wide.  The boxes are inflated by 2^-21 of the scene's bound (2.9e-5 under the dome),
    so the hundreds of spheres smaller than that share one box about the origin; from 2e-4 away a pixel is 1e-6 wide there, and every camera ray
    (the lens is 1e-5 wide) passes through that box: it descends the deep side of every node first, the sibling left on the stack, down to the
    deepest leaves, before it reaches the spheres it can see.  (Under the dome the camera's position does not change the scene's bound, so the
    tree is the one of HOST_TABLE.)"""
    return scene(items, lens, lookfrom=CHAIN_CAMERA_AT, lookat=(4.0, 0.0, 0.0), vfov=6.0, aperture=2e-5, focus_dist=2.0)


# spheres that cannot be bounded (non-finite coordinates, coordinates beyond 1e15), as [cx, cy, cz, r] rows: the builder keeps them out of the tree
UNBOUNDABLE = np.array([[np.inf, 0, 0, 1.0], [0, -np.inf, 0, 1.0], [np.nan, 0, 0, 1.0], [0, 0, 0, np.inf], [0, 0, 0, np.nan], [1e16, 0, 0, 1.0],
                        [0, 0, -3e15, 1.0], [0, 0, 0, 2e15], [0, 0, 0, -np.inf]])


def scene_sized(n):
    """[n, 4]: n spheres of one size, each as large as the scene -- from the seventeenth on they go into the tree (the cap on big primitives)"""
    return np.array([[0.1 * k, 0.0, 0.0, 50.0] for k in range(n)])


def sphere_geom(items):
    """[n, 4] cx cy cz r of a list of plain spheres: what rtmi_test_build_tree takes"""
    return np.ascontiguousarray([[it.center[0], it.center[1], it.center[2], it.radius] for it in items], np.float64)


# ---- the chains ------------------------------------------------------------------------------------------------------------------------------
def chain_geom(n, q, rho):
    k = np.arange(n, dtype=np.float64)
    return 4.0 * q ** k, rho * q ** k


def chain(n, q, rho, dome=True):
    """spheres of centre (4 q^k, 0, 0) and radius rho q^k, k = 0 .. n-1, behind a radius-60 light about the origin (the one big primitive)"""
    H = _mods()[0]
    mats, light = _materials()
    cx, rad = chain_geom(n, q, rho)
    items = [_dome(light)] if dome else []
    items += [H.sphere(center=np.array([cx[k], 0.0, 0.0]), radius=rad[k], material=mats[k % 3]) for k in range(n)]
    return items


def chain_ext(n, q, rho):
    """the chain with every fifth item of another kind at the same place and scale -- rect_xy, triangle, box, translate(rotate_y(sphere)) in
    turn --, which sends the scene to the mixed-kind kernels"""
    H = _mods()[0]
    mats, light = _materials()
    cx, rad = chain_geom(n, q, rho)
    items = [_dome(light)]
    for k in range(n):
        c, s, m = np.array([cx[k], 0.0, 0.0]), rad[k], mats[k % 3]
        if k % 5 != 4:
            items.append(H.sphere(center=c, radius=s, material=m))
            continue
        kind = (k // 5) % 4
        if kind == 0:
            items.append(H.rect_xy(x0=c[0] - s, y0=-s, x1=c[0] + s, y1=s, k=0.0, material=m))
        elif kind == 1:
            items.append(H.triangle(v0=c + np.array([-s, -s, 0.0]), v1=c + np.array([s, -s, 0.5 * s]), v2=c + np.array([0.0, s, -0.5 * s]), material=m))
        elif kind == 2:
            items.append(H.box(p0=c - 0.7 * s, p1=c + 0.7 * s, material=m))
        else:  # a sphere about the origin, turned (which leaves it where it is) and moved into place
            items.append(H.translate(item=H.rotate_y(item=H.sphere(center=np.zeros(3), radius=s, material=m), theta=30.0), offset=c))
    return items


def chain_rays(n, q, rho, count, seed, n_fallback=300):
    """-> (rays [count + n_fallback, 7], number of fallback rays at the end).  Every ray is aimed at a sphere k of the chain and passes its centre
    at a distance drawn from {0, r/2, r (1 - 1e-12), r (1 + 1e-12), r (1 - 1e-6)}.  Half travel towards -x and start outside, so that they meet
    the shallow leaves first; half travel towards +x and start beyond the small end (x < 0), so that they descend the deep side first while
    every sibling box on the way is pushed.  Start distances r {1.5, 20, 1e4} + {0, 5}, for the +x rays measured beyond x = 0.  All directions
    are oblique; the last n_fallback rays are copies of the first with d.y = 0 (not boundable in float: the exact flat-scan fallback)."""
    rng = np.random.default_rng(seed)
    cx, rad = chain_geom(n, q, rho)
    k = rng.integers(0, n, count)
    c, r = cx[k], rad[k]
    off = r * rng.choice([0.0, 0.5, 1.0 - 1e-12, 1.0 + 1e-12, 1.0 - 1e-6], count)
    plus = np.arange(count) % 2 == 1
    d = np.stack([np.where(plus, 1.0, -1.0), rng.choice([-1.0, 1.0], count) * rng.uniform(0.05, 0.6, count),
                  rng.choice([-1.0, 1.0], count) * rng.uniform(0.05, 0.6, count)], axis=1)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    # a unit vector across the direction, turned by a random angle about it
    e1 = np.cross(d, np.array([0.0, 1.0, 0.0])); e1 /= np.linalg.norm(e1, axis=1, keepdims=True)
    e2 = np.cross(d, e1)
    phi = rng.uniform(0.0, 2.0 * np.pi, count)
    p = np.stack([c, np.zeros(count), np.zeros(count)], axis=1) + off[:, None] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
    s = r * rng.choice([1.5, 20.0, 1e4], count) + rng.choice([0.0, 5.0], count)
    dist = np.where(plus, (p[:, 0] + s) / d[:, 0], s)
    o = p - d * dist[:, None]
    rays = np.concatenate([o, d * rng.choice([1.0, 3.0], count)[:, None], np.zeros((count, 1))], axis=1)
    fb = rays[:n_fallback].copy()
    fb[:, 4] = 0.0
    return np.concatenate([rays, fb]), n_fallback


# ---- degenerate input ------------------------------------------------------------------------------------------------------------------------
def _bystanders(mats, count=12, seed=5):
    H = _mods()[0]
    rng = np.random.default_rng(seed)
    return [H.sphere(center=np.array([1.5, 0.0, 0.0]) + rng.normal(0, 2.5, 3), radius=float(rng.uniform(0.1, 0.4)), material=mats[k % 3]) for k in range(count)]


def identical(n, bystanders=0, dome=True):
    """n spheres of one centre and one radius (every leaf ties exactly; the materials differ, so the winner shows)"""
    H = _mods()[0]
    mats, light = _materials()
    items = [H.sphere(center=np.array([1.5, 0.0, 0.0]), radius=0.75, material=mats[k % 3]) for k in range(n)]
    items += _bystanders(mats, bystanders)
    return items + ([_dome(light)] if dome else [])


def shells(n, dome=True):
    """n concentric spheres, radius 0.2 .. 1.0 ascending with the index"""
    H = _mods()[0]
    mats, light = _materials()
    items = [H.sphere(center=np.array([1.5, 0.0, 0.0]), radius=0.2 + 0.8 * k / (n - 1), material=mats[k % 3]) for k in range(n)]
    return items + ([_dome(light)] if dome else [])


def many_big(n_big, n_small, seed=7):
    """n_big concentric shells of radius 60 .. 40, descending with the index, around a cloud of n_small small spheres: the builder keeps the first
    sixteen out of the tree and the others go INTO it, each with a box the size of the scene.  Those are the innermost four: three of glass and,
    behind them, the light -- what a path from the cloud meets on its way out is decided inside the tree."""
    H, S, T, _ = _mods()
    mats, light = _materials()
    glass = S.dielectric(ri=1.5)
    items = [H.sphere(center=np.zeros(3), radius=60.0 - 20.0 * k / (n_big - 1), material=light if k == n_big - 4 else glass) for k in range(n_big)]
    rng = np.random.default_rng(seed)
    items += [H.sphere(center=np.array([1.5, 0.0, 0.0]) + rng.normal(0, 3.0, 3), radius=float(rng.uniform(0.05, 0.5)), material=mats[k % 3]) for k in range(n_small)]
    return items


def negative_radius(n, seed=11):
    """a random cloud, every second sphere with radius < 0 (hitable.clj divides by the radius: the normal points inward), glass and lambertian"""
    H = _mods()[0]
    mats, light = _materials()
    rng = np.random.default_rng(seed)
    items = [_dome(light)]
    for k in range(n):
        rad = float(rng.uniform(0.1, 0.6)) * (-1.0 if k % 2 else 1.0)
        items.append(H.sphere(center=np.array([1.5, 0.0, 0.0]) + rng.normal(0, 2.0, 3), radius=rad, material=mats[2 if k % 4 < 2 else 0]))
    return items


def zero_radius(n, seed=13):
    """n spheres of radius 0 among a dozen ordinary ones"""
    H = _mods()[0]
    mats, light = _materials()
    rng = np.random.default_rng(seed)
    items = [_dome(light)]
    items += [H.sphere(center=np.array([1.5, 0.0, 0.0]) + rng.normal(0, 2.0, 3), radius=0.0 if k % 2 == 0 else -0.0, material=mats[k % 3]) for k in range(n)]
    return items + _bystanders(mats, 12, seed)


# ---- the chooser's thresholds ----------------------------------------------------------------------------------------------------------------
def cloud(n, seed=17, dome=True):
    """n small spheres in a cube: n - 1 inner nodes, no entry grid below 256"""
    H = _mods()[0]
    mats, light = _materials()
    rng = np.random.default_rng(seed)
    items = [H.sphere(center=np.array([1.5, 0.0, 0.0]) + rng.uniform(-3.0, 3.0, 3), radius=0.2, material=mats[k % 3]) for k in range(n)]
    return items + ([_dome(light)] if dome else [])


def layer(n, seed=19, dome=True):
    """n spheres of radius 0.2 standing on a 20 x 20 square: from 256 on the builder lays an entry grid over them"""
    H = _mods()[0]
    mats, light = _materials()
    rng = np.random.default_rng(seed)
    xz = rng.uniform(-10.0, 10.0, (n, 2))
    items = [H.sphere(center=np.array([xz[k, 0], 0.2, xz[k, 1]]), radius=0.2, material=mats[k % 3]) for k in range(n)]
    return items + ([_dome(light)] if dome else [])


def mixed(n, seed=23):
    """a mixed-kind world of exactly n primitives (spheres, rectangles, triangles; the first a light): 64 is the last size the small-world scan takes"""
    H = _mods()[0]
    mats, light = _materials()
    rng = np.random.default_rng(seed)
    items = [_dome(light)]
    for k in range(1, n):
        c, m = np.array([1.5, 0.0, 0.0]) + rng.normal(0, 2.0, 3), mats[k % 3]
        if k % 3 == 0:
            items.append(H.rect_xz(x0=c[0] - 0.5, z0=c[2] - 0.4, x1=c[0] + 0.5, z1=c[2] + 0.4, k=c[1], material=m))
        elif k % 3 == 1:
            items.append(H.triangle(v0=c, v1=c + rng.normal(0, 0.6, 3), v2=c + rng.normal(0, 0.6, 3), material=m))
        else:
            items.append(H.sphere(center=c, radius=0.3, material=m))
    return items


def cloud_rays(count, seed, spread=4.0):
    """rays from around CAMERA_AT and from inside the cloud about (1.5, 0, 0), towards it"""
    rng = np.random.default_rng(seed)
    o = np.where(rng.random((count, 1)) < 0.5, np.array(CAMERA_AT) + rng.normal(0, 0.5, (count, 3)), np.array([1.5, 0.0, 0.0]) + rng.normal(0, 1.5, (count, 3)))
    d = np.array([1.5, 0.0, 0.0]) + rng.normal(0, spread, (count, 3)) - o
    return np.concatenate([o, d, rng.random((count, 1))], axis=1)
