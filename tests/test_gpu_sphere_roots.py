"""The exact sphere test's roots (rtmi_device.h: sphere_roots, sphere_roots_any_order, exact_prim_test, exact_prim_test_lane): a lane whose
origin is inside or on the sphere forms the second root directly, the second-root arm is entered on `!(t > t-min)` alone, the leaf's record
is fetched at a 32-bit offset and its tie rule sits behind `t < best`.  None of it may change a result: on rays aimed at the places where the forms decide -- origins
inside, on and just outside a surface, heading in, out and along it, `oc` perpendicular to `d`, `(oc.d)^2` underflowing, one lane per wave
on the IEEE division -- and over the intervals that switch the selector's conditions off one by one, the device's closest hit equals the CPU
oracle's in hit flag, primitive index and t, bit for bit, for the tree and for the Hitlist scans, static and moving, in both precisions."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raytrace_clj_amd as r
from raytrace_clj_amd import core
from raytrace_clj_amd import flatten as fl

FLT_MAX = 3.4028234663852886e38
WAVES = 100  # 64 x 100 rays per case
INTERVALS = [
    (0.001, FLT_MAX),   # a render's
    (0.0, FLT_MAX),     # t-min below 2^-300: the per-ray reciprocal is off, every lane divides
    (1e-310, FLT_MAX),  # the same with a t-min that is not zero
    (-1.0, FLT_MAX),    # no behind-the-origin early-out, no selector
    (0.001, 1.2),       # t-max between the two roots of the rays of family 7 (|d| = 1) ...
    (0.001, 0.9),       # ... and below their first root: it passes t-min and fails t-max, and so must the second
]


def _unit(v):
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _two_moving_big():
    """a ground and a dome that both move during the shutter (the big primitives' moving arm), over a few small spheres"""
    H, S, T = r.hitable, r.shader, r.texture
    vec3 = lambda *a: np.array(a, np.float64)  # noqa: E731
    mat = S.lambertian(albedo=T.constant(color=vec3(0.5, 0.5, 0.5)))
    rng = np.random.default_rng(5)
    items = [H.moving_sphere(center0=vec3(0, 0, 0), t0=0.0, center1=vec3(0.5, 0.25, 0), t1=1.0, radius=1000, material=mat),
             H.moving_sphere(center0=vec3(0, -1000, 0), t0=0.0, center1=vec3(0, -1000.5, 0.25), t1=1.0, radius=1000, material=mat)]
    for k in range(30):
        c = vec3(rng.uniform(-6, 6), 0.2, rng.uniform(-6, 6))
        if k % 3 == 0:
            items.append(H.moving_sphere(center0=c, t0=0.0, center1=c + vec3(0, 0.3 * rng.random(), 0), t1=1.0, radius=0.2, material=mat))
        else:
            items.append(H.sphere(center=c, radius=0.2, material=mat))
    cam = r.camera.thin_lens_camera(lookfrom=vec3(13, 2, 3), lookat=vec3(0, 0, 0), vup=vec3(0, 1, 0), vfov=20, aspect=2.0, aperture=0.0,
                                    focus_dist=10.0, t0=0.0, t1=1.0)
    return {"camera": cam, "world": H.hitlist(items=items)}


# name -> (scene, accel option, scan variants): the make-bvh worlds run the device's tree, the Hitlists the ordered scans (1, 2: sphere_roots
# from LDS and from scalar registers; 3: the culled scan, exact_prim_test)
SCENES = {
    "tree": (lambda: r.scene.make_random_scene(64, 32, 3, False), 1, (None,)),
    "tree-moving": (lambda: r.scene.make_random_scene(64, 32, 3, True), 1, (None,)),
    "hitlist": (lambda: r.scene.make_random_scene(64, 32, 3, False, bvh=False), 0, (1, 2, 3)),
    "hitlist-moving": (lambda: r.scene.make_random_scene(64, 32, 3, True, bvh=False), 0, (1, 2, 3)),
    "two-moving-big": (_two_moving_big, 1, (None,)),
}


def ieee_lane(n):
    """one lane of every wave, another one from wave to wave (so that it falls on every family and target)"""
    i = np.arange(n)
    return i % 64 == (13 * (i // 64) + 5) % 64


def probe_rays(f, seed):
    """64 x WAVES rays in eight families around a small sphere, a sphere of radius 1 and the two spheres of radius 1000 of the scene, each at
    its place at the ray's time; |d| cycles through 1e-3, 1, 1e3, and one lane of every wave is at 1e-120 or 1e120"""
    rng = np.random.default_rng(seed)
    n = 64 * WAVES
    g = f.prim_geom
    small = np.flatnonzero(g[:, 3] < 0.5)
    targets = np.concatenate([[0, 1], np.flatnonzero((g[:, 3] >= 0.5) & (g[:, 3] < 50))[:1], small[:5]])
    tgt = targets[np.arange(n) % len(targets)]
    time = rng.random(n)
    frac = ((time - g[tgt, 7]) / (g[tgt, 8] - g[tgt, 7]))[:, None]
    c = g[tgt, 0:3] * (1.0 - frac) + g[tgt, 4:7] * frac
    rad = g[tgt, 3:4]
    u = _unit(rng.normal(size=(n, 3)))
    w = _unit(np.cross(u, rng.normal(size=(n, 3))))  # perpendicular to u
    fam = (np.arange(n) // len(targets)) % 8
    heading = (np.arange(n) // (8 * len(targets))) % 3  # in, out, along the surface
    o = np.zeros((n, 3))
    d = np.zeros((n, 3))
    lean = rng.uniform(0.0, 0.8, (n, 1))
    dirs = [_unit(-u + lean * w), _unit(u + lean * w), w]
    any_dir = np.where(heading[:, None] == 0, dirs[0], np.where(heading[:, None] == 1, dirs[1], dirs[2]))
    scale = np.array([1e-3, 1.0, 1e3])[(np.arange(n) // 7) % 3][:, None]
    # 0: strictly inside
    k = fam == 0
    o[k] = (c + rad * rng.uniform(0.0, 0.99, (n, 1)) * u)[k]
    d[k] = any_dir[k]
    # 1: on the surface, as c + r u (cq a few ulps either side of 0), heading in, out and along it
    k = fam == 1
    o[k] = (c + rad * u)[k]
    d[k] = any_dir[k]
    # 2: outside, within t-min |d| of the surface, heading in: the first root is below t-min = 0.001 (the fallback arm)
    k = fam == 2
    o[k] = (c + (rad + 0.3 * 0.001 * scale) * u)[k]
    d[k] = dirs[0][k]
    # 3: outside, heading away (the early-out) and along the surface
    k = fam == 3
    o[k] = (c + rad * rng.choice([1.0 + 1e-9, 1.01, 1.5], (n, 1)) * u)[k]
    d[k] = np.where(heading[:, None] == 0, dirs[2], dirs[1])[k]
    # 4: oc perpendicular to d exactly: oc = (s, 0, 0), d along y or z; s inside, on and outside the sphere
    k = fam == 4
    s = rad * rng.choice([0.0, 0.5, 1.0, -1.0, 1.0 + 1e-12, 2.0], (n, 1))
    o[k] = (c + s * np.array([1.0, 0.0, 0.0]))[k]
    d[k] = np.where(heading[:, None] == 0, [0.0, 1.0, 0.0], np.where(heading[:, None] == 1, [0.0, 0.0, -1.0], [0.0, -1.0, 0.0]))[k]
    # 5: d = (+-2^-600, +-1, 0) against oc = (s, 0, 0): (oc.d)^2 underflows to zero.  (Not to a denormal: there the kernels' reduced quadratic and the
    # reference's literal one round differently -- scaling by 4 no longer commutes with rounding -- which is outside the parity contract, rtmi_device.h)
    k = fam == 5
    o[k] = (c + s * np.array([1.0, 0.0, 0.0]))[k]
    d[k] = np.where(heading[:, None] == 0, [2.0 ** -600, 1.0, 0.0], np.where(heading[:, None] == 1, [-2.0 ** -600, 1.0, 0.0], [2.0 ** -600, -1.0, 0.0]))[k]
    # 6: from far outside, through the sphere: both roots in front
    k = fam == 6
    o[k] = (c + rad * rng.uniform(1.5, 4.0, (n, 1)) * u)[k]
    d[k] = dirs[0][k]
    # 7: at distance 1 from the surface, straight at the centre: roots 1 / |d| and (1 + 2 r) / |d|
    k = fam == 7
    o[k] = (c + (rad + 1.0) * u)[k]
    d[k] = -u[k]
    d *= scale
    lane = ieee_lane(n)
    d[lane] *= np.where((np.arange(n) // 64) % 2 == 0, 1e-120, 1e120)[lane][:, None]
    return np.concatenate([o, d, time[:, None]], axis=1)


_CASES = {}


def case(name, oracles):
    """the flattened scene, its rays and the oracle's answers per precision and interval: computed once, shared, never changed"""
    if name not in _CASES:
        flat = fl.flatten(SCENES[name][0]())
        rays = probe_rays(flat, 31)
        ref = {}
        for prec in ("f64", "f32"):
            for iv in INTERVALS:
                a = oracles[prec].probe_hit(flat, rays, tmin=iv[0], tmax=iv[1])[:, :3]
                a.setflags(write=False)
                ref[prec, iv] = a
        _CASES[name] = (flat, rays, ref)
    return _CASES[name]


def test_the_rays_reach_every_arm(oracle, oracle_f32):
    """the families are about what they say: inside and on-surface origins hit, the fallback family's hit is the far side of its sphere under the
    render's t-min and the near side under t-min = 0, the early-out family mostly leaves its sphere behind"""
    flat, rays, ref = case("tree", {"f64": oracle, "f32": oracle_f32})
    n = len(rays)
    fam = (np.arange(n) // 8) % 8  # (this scene has eight targets)
    lane = ieee_lane(n)
    a, b = ref["f64", INTERVALS[0]], ref["f64", INTERVALS[1]]
    assert a[(fam == 0) & ~lane, 0].all(), "a ray from inside a sphere hits it"
    k = (fam == 2) & ~lane
    assert (b[k, 0] == 1).all() and (a[k, 2] > b[k, 2]).mean() > 0.9, "the near root is below t-min = 0.001 and above 0"
    k = (fam == 7) & ~lane
    assert (ref["f64", INTERVALS[5]][k, 0] == 0).mean() > 0.3, "t-max below the first root"


@pytest.mark.parametrize("precision", ["f64", "f32"])
@pytest.mark.parametrize("name", sorted(SCENES))
def test_closest_hits_equal_the_oracle(name, precision, oracle, oracle_f32):
    flat, rays, ref = case(name, {"f64": oracle, "f32": oracle_f32})
    _, accel, variants = SCENES[name]
    ctx = core.Context(0)
    ctx.set_option("accel", accel)
    ds = core.DeviceScene(flat, ctx=ctx)
    try:
        if name == "two-moving-big":
            assert ds.tree_info()[3] == 2, "both moving spheres of radius 1000 are big primitives"
        for variant in variants:
            if variant is not None:
                ctx.set_option("scan_variant", variant)
            for iv in INTERVALS:
                got = ds.probe_hit(rays, iv[0], iv[1], precision=precision)[:, :3]
                exp = ref[precision, iv]
                bad = np.flatnonzero((got != exp).any(axis=1))
                print(name, precision, variant, iv, "hits", int(exp[:, 0].sum()), "differ", len(bad))
                assert len(bad) == 0, (name, precision, variant, iv, len(bad), bad[:8].tolist(), got[bad[:4]].tolist(), exp[bad[:4]].tolist())
    finally:
        ds.close(); ctx.close()


@pytest.mark.parametrize("lds_stash,defer", [(1, 1), (0, 1), (1, 0), (0, 0)])
def test_frames_of_the_sphere_kernels(lds_stash, defer, oracle, cover11_moving, monkeypatch):
    """one 64 x 32 x 4 frame of the time-sliced sphere kernels (camera-ray stash in LDS and in registers, with and without the deferring twin)
    against the oracle: counters equal, pixels within the images' tolerance"""
    nx, ny, ns = 64, 32, 4
    key = "frame"
    if key not in _CASES:
        _CASES[key] = oracle.render(fl.flatten(cover11_moving), nx, ny, ns, 50, core.RENDER_SEED, nthreads=8)
    exp, exp8, ecnt = _CASES[key]
    monkeypatch.setenv("RTMI_SPHERE_LDS_STASH", str(lds_stash))
    ctx = core.Context(0)
    ctx.set_option("defer_emitters", defer)
    ds = core.DeviceScene(fl.flatten(cover11_moving), ctx=ctx)
    try:
        lin, q, cnt = ds.render(nx, ny, ns)
        err = float(np.sqrt(np.mean((lin - exp) ** 2)))
        print("lds stash", lds_stash, "defer", defer, "pixel RMS", err)
        assert np.array_equal(cnt, ecnt), (cnt, ecnt)
        assert err <= 1e-4, err
    finally:
        ds.close(); ctx.close()
