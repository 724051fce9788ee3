"""Shared by test_frame_reference.py (CPU) and test_gpu_frame_exact.py (GPU): scenes whose colours never touch libm, every sample of a
pinhole frame taken from the oracle's probes, and numpy restatements of the back half of a frame -- the in-order fold of core.clj:52-53,
the 8-bit quantiser of core.clj:54-56, the tile dealing of rtmi_assemble_device, the standard error of the mean.  Nothing here imports the
device library; the oracle is passed in.  Not a test module (pytest collects test_*.py only)."""
import numpy as np

import raytrace_clj_amd as r
from raytrace_clj_amd import flatten as fl
from raytrace_clj_amd.util import vec3

H, S, T = r.hitable, r.shader, r.texture
SEED = 0x5EED0002  # core.RENDER_SEED
DEPTH = 50
REAL = {"f64": np.float64, "f32": np.float32}


# ---- scenes: + - * / sqrt, floor and integer work only from the camera to the 8-bit value ---------------------------------------------
def _camera(nx, ny, lookfrom, lookat, vfov, lens):
    kw = dict(lookfrom=lookfrom, lookat=lookat, vup=vec3(0, 1, 0), vfov=vfov, aspect=nx / ny)
    if not lens:
        return r.camera.pinhole_camera(**kw)
    return r.camera.thin_lens_camera(aperture=0.3, focus_dist=10.0, t0=0.0, t1=1.0, **kw)


def sphere_scene(nx, ny, lens=False):
    """Spheres and moving spheres with constant textures, no constant background: the "sky" is 120 large emissive spheres of different colours on
    a shell around the scene, the ground a fuzzy metal, 60 small lambertian / metal / emissive spheres (every fifth moving), camera looking down.
    Runs in f32 as well (no rectangles, instances or procedural textures).  -> FlatScene"""
    rng = np.random.default_rng(1)
    items = [H.sphere(center=vec3(0, -100.5, 0), radius=100.0, material=S.metal(albedo=T.constant(color=vec3(0.8, 0.7, 0.6)), fuzz=0.6))]
    for k in range(120):
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        items.append(H.sphere(center=vec3(*(d * 60.0)), radius=14.0, material=S.diffuse_light(tex=T.constant(color=vec3(*(rng.random(3) * 2.0))))))
    for k in range(60):
        c = vec3(rng.uniform(-5, 5), rng.uniform(-0.3, 1.5), rng.uniform(-5, 5))
        m = [S.lambertian(albedo=T.constant(color=vec3(*rng.random(3)))), S.metal(albedo=T.constant(color=vec3(*rng.random(3))), fuzz=float(rng.choice([0.0, 0.4]))),
             S.diffuse_light(tex=T.constant(color=vec3(4, 3, 2)))][k % 3]
        if k % 5 == 0:
            items.append(H.moving_sphere(center0=c, t0=0.0, center1=c + vec3(0, 0.3, 0), t1=1.0, radius=0.35, material=m))
        else:
            items.append(H.sphere(center=c, radius=0.35, material=m))
    # looking down steeply: with more of the shell in direct view too many pixels see one light in every sample (test_frame_reference.py holds the cap)
    return fl.flatten({"camera": _camera(nx, ny, vec3(0, 8, 7), vec3(0, 0, 0), 35, lens), "world": H.hitlist(items=items)})


def mixed_scene(nx, ny):
    """Every libm-free record kind under make_bvh: a Perlin-turbulence light as the sky and a Perlin-turbulence ground, boxes (plain, translated,
    rotated), triangles, rectangles of the three orientations (one with flipped normals, one emissive with radiance far above 1, one with an image
    map, whose uv on a rectangle is linear), spheres and moving spheres.  f64 only.  -> FlatScene with the nested world for the oracle"""
    from oracle.tree import attach_tree
    rng = np.random.default_rng(2)
    items = [H.sphere(center=vec3(0, 0, 0), radius=500.0, material=S.diffuse_light(tex=T.perlin_turbulence(scale=0.02, depth=3))),
             H.sphere(center=vec3(0, -100.5, 0), radius=100.0, material=S.lambertian(albedo=T.perlin_turbulence(scale=2.0, depth=2))),
             H.rect_xz(x0=-1.5, z0=-1.5, x1=1.5, z1=1.5, k=3.5, material=S.diffuse_light(tex=T.constant(color=vec3(15, 12, 9)))),
             H.flip_normals(item=H.rect_yz(y0=-0.5, z0=-3, y1=2.5, z1=3, k=4.5, material=S.metal(albedo=T.constant(color=vec3(0.9, 0.9, 0.8)), fuzz=0.0))),
             H.rect_xy(x0=-4, y0=-0.5, x1=-1, y1=1.5, k=-3.5, material=S.lambertian(albedo=T.image_map(image=r.scene.synthetic_earth(64, 32)))),
             H.rect_yz(y0=-0.5, z0=-2, y1=1.0, z1=1, k=-4.5, material=S.lambertian(albedo=T.perlin_noise(scale=3.0)))]
    for k in range(30):
        c = vec3(rng.uniform(-4, 4), rng.uniform(-0.3, 1.5), rng.uniform(-4, 4))
        m = [S.lambertian(albedo=T.constant(color=vec3(*rng.random(3)))), S.metal(albedo=T.constant(color=vec3(*rng.random(3))), fuzz=float(rng.choice([0.0, 0.4]))),
             S.diffuse_light(tex=T.constant(color=vec3(4, 3, 2)))][k % 3]
        kind = k % 6
        if kind == 0:
            items.append(H.box(p0=c, p1=c + vec3(0.6, 0.7, 0.5), material=m))
        elif kind == 1:
            items.append(H.triangle(v0=c, v1=c + vec3(1, 0, 0.2), v2=c + vec3(0.1, 1, 0), material=m))
        elif kind == 2:
            items.append(H.translate(item=H.rotate_y(item=H.box(p0=vec3(0, 0, 0), p1=vec3(0.5, 0.8, 0.5), material=m), theta=33.0), offset=c))
        elif kind == 3:
            items.append(H.moving_sphere(center0=c, t0=0.0, center1=c + vec3(0, 0.3, 0), t1=1.0, radius=0.3, material=m))
        elif kind == 4:
            items.append(H.translate(item=H.sphere(center=vec3(0, 0, 0), radius=0.35, material=m), offset=c))
        else:
            items.append(H.sphere(center=c, radius=0.3, material=m))
    world = H.make_bvh(items, 0.0, 1.0)
    flat = fl.flatten({"camera": _camera(nx, ny, vec3(0, 2, 9), vec3(0, 0.3, 0), 50, False), "world": world})
    return attach_tree(flat, world)


def constant_light_scene(color):
    """the camera inside one DiffuseLight sphere of constant colour: every sample of every pixel is `color` (one segment), so the mean is
    (c + ... + c) * (1 / ns) and the quantisers behind render(region=) and render_progressive can be driven with chosen values"""
    cam = r.camera.pinhole_camera(lookfrom=vec3(0, 0, 0), lookat=vec3(0, 0, -1), vup=vec3(0, 1, 0), vfov=90, aspect=2.0)
    light = S.diffuse_light(tex=T.constant(color=np.asarray(color, np.float64)))
    return fl.flatten({"camera": cam, "world": H.hitlist(items=[H.sphere(center=vec3(0, 0, 0), radius=100.0, material=light)])})


# ---- the render stream, restated with numpy integers (rt_oracle.c: mix64, rto_sample_key, rng_next) -------------------------------------
_GOLD = np.uint64(0x9E3779B97F4A7C15)
_MUL = np.uint64(0xD6E8FEB86659FD93)
_STEP = np.uint64(0xD1B54A32D192ED03)


def _mix64(z):
    s = np.uint64(32)
    z = z ^ (z >> s)
    z = z * _MUL
    z = z ^ (z >> s)
    z = z * _MUL
    return z ^ (z >> s)


def sample_keys(seed, pixel, sample):
    """stream keys of (seed, pixel index j * nx + i, sample), arrays of uint64"""
    with np.errstate(over="ignore"):
        pixel, sample = np.asarray(pixel, np.uint64), np.asarray(sample, np.uint64)
        return _mix64(_mix64(np.uint64(seed) ^ (_GOLD * (pixel + np.uint64(1)))) + _STEP * (sample + np.uint64(1)))


def draws(keys, d, precision):
    """draw number d of every stream: 53 random bits * 2^-53 in f64, 24 bits * 2^-24 in f32 (both exact)"""
    with np.errstate(over="ignore"):
        z = _mix64(keys + _GOLD * np.uint64(d + 1))
    if precision == "f32":
        return (z >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return (z >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


# ---- every sample of a pinhole frame on its own --------------------------------------------------------------------------------------------
def frame_samples(oracle, flat, nx, ny, ns, seed=SEED, depth=DEPTH):
    """-> (samples [nx, ny, ns, 3] in the oracle's precision, indexed [i, j, s, c] in reference coordinates (j = 0 at the bottom), segments of every sample [nx, ny, ns]).
    pixel() of rt_oracle.c for a camera that draws nothing: u = (R(float(i)) + draw 0) / R(nx), v likewise with draw 1, the ray from
    probe_camera, its colour from probe_paths with the stream continuing at draw 2."""
    assert int(flat.cam_kind) == 0, "a thin lens draws inside get-ray: its samples cannot be rebuilt from the probes"
    R = REAL[oracle.precision]
    ii, jj, ss = (a.ravel() for a in np.meshgrid(np.arange(nx), np.arange(ny), np.arange(ns), indexing="ij"))
    keys = sample_keys(seed, jj * nx + ii, ss)
    u = (ii.astype(np.float32).astype(R) + draws(keys, 0, oracle.precision)) / R(nx)
    v = (jj.astype(np.float32).astype(R) + draws(keys, 1, oracle.precision)) / R(ny)
    assert u.dtype == R and v.dtype == R
    cam = oracle.probe_camera(flat, np.stack([u, v], 1).astype(np.float64), keys)
    assert (cam[:, 7] == 0).all()  # no draws consumed
    rgb, nseg, _, _ = oracle.probe_paths(flat, cam[:, :7], keys, depth=depth, ctr0=2, max_seg=0)
    smp = rgb.reshape(nx, ny, ns, 3)
    assert np.array_equal(smp.astype(R).astype(np.float64), smp)  # the probe hands out values of R, widened
    return smp.astype(R), nseg.reshape(nx, ny, ns)


# What the two test modules run: every scene at SIZE with ns in NS_EDGE (once, the edges of the fold: no addition, one addition) and NS_FOLD (odd,
# > 4: where the order of the additions shows), and at SIZE_PASSES[scene] with ns = 13, a frame of enough tiles for option "workspace_bytes" at its
# floor of 1 MiB to split 13 samples into >= 3 passes.  No size is a multiple of 8 in either direction.
SCENES = {"spheres": sphere_scene, "spheres-lens": lambda nx, ny: sphere_scene(nx, ny, True), "mixed": mixed_scene}
PRECISIONS = {"spheres": ("f64", "f32"), "spheres-lens": ("f64", "f32"), "mixed": ("f64",)}
SIZE = (61, 37)
SIZE_PASSES = {"spheres": (203, 99), "spheres-lens": (203, 99), "mixed": (117, 93)}
NS_EDGE, NS_FOLD, NS_MAX = (1, 2), (7, 13), 13
CASES = [(name, p) for name in SCENES for p in PRECISIONS[name]]
_scenes, _samples = {}, {}


def scene(name, nx, ny):
    if (name, nx, ny) not in _scenes:
        _scenes[name, nx, ny] = SCENES[name](nx, ny)
    return _scenes[name, nx, ny]


def samples(oracle, name, nx, ny, ns):
    """frame_samples of a named scene, the first ns <= NS_MAX samples (a stream is keyed by the sample's index, not by ns: one reconstruction serves
    every ns) -> (samples [nx, ny, ns, 3], total segments of those samples)"""
    key = (oracle.precision, name, nx, ny)
    if key not in _samples:
        _samples[key] = frame_samples(oracle, scene(name, nx, ny), nx, ny, NS_MAX)
    smp, nseg = _samples[key]
    return smp[:, :, :ns], int(nseg[:, :, :ns].sum())


def to_image(a):
    """[i, j, c] in reference coordinates -> [row, column, c] doubles, row 0 = top (core.clj:105)"""
    return np.ascontiguousarray(np.transpose(a, (1, 0, 2))[::-1]).astype(np.float64)


def _add(a, b):
    out = a + b
    assert out.dtype == a.dtype  # the fold stays in the frame's precision
    return out


def fold_in_order(smp, first=0, last=None):
    """core.clj:52-53 restated: start FROM sample `first`, add the next ones one at a time, in order"""
    last = smp.shape[2] if last is None else last
    acc = smp[:, :, first].copy()
    for s in range(first + 1, last):
        acc = _add(acc, smp[:, :, s])
    return acc


def mean_of(acc, ns):
    """(mul (/ 1.0 nr)): the sum times the reciprocal, both in the frame's precision"""
    R = acc.dtype.type
    out = acc * (R(1.0) / R(ns))
    assert out.dtype == acc.dtype
    return out


def frame_in_order(smp, ns=None):
    """the frame the back half must produce from these samples (the first ns of them): [row, column, c] doubles"""
    ns = smp.shape[2] if ns is None else ns
    return to_image(mean_of(fold_in_order(smp, 0, ns), ns))


# the same samples folded WRONGLY: what a fold that is not the reference's would return
def frame_reversed(smp):
    return to_image(mean_of(fold_in_order(smp[:, :, ::-1]), smp.shape[2]))


def frame_pairwise(smp):
    parts = [smp[:, :, s] for s in range(smp.shape[2])]
    while len(parts) > 1:
        nxt = [_add(parts[k], parts[k + 1]) for k in range(0, len(parts) - 1, 2)]
        if len(parts) % 2:
            nxt.append(parts[-1])
        parts = nxt
    return to_image(mean_of(parts[0], smp.shape[2]))


def frame_divided(smp):
    acc = fold_in_order(smp)
    out = acc / acc.dtype.type(smp.shape[2])
    assert out.dtype == acc.dtype
    return to_image(out)


def frame_restarted(smp, per_pass):
    """a fold split into sample passes of `per_pass` that restarts at a pass boundary instead of carrying: only the last pass survives"""
    ns = smp.shape[2]
    first = ((ns - 1) // per_pass) * per_pass
    return to_image(mean_of(fold_in_order(smp, first, ns), ns))


WRONG_FOLDS = {"reversed": frame_reversed, "pairwise": frame_pairwise, "sum / ns": frame_divided,
               "restart, passes of 2": lambda smp: frame_restarted(smp, 2), "restart, passes of 4": lambda smp: frame_restarted(smp, 4)}


def share_changed(img, ref):
    """share of the pixels in which any channel differs"""
    return float((img != ref).any(axis=2).mean())


def share_all_equal(smp):
    """share of the pixels whose samples are all equal"""
    return float((smp == smp[:, :, :1]).all(axis=(2, 3)).mean())


def stderr_two_pass(smp, k):
    """float64 two-pass standard error of the mean over the first k samples, the largest of the three channels; [row, column]; +inf at k = 1"""
    x = smp[:, :, :k].astype(np.float64)
    if k == 1:
        return np.full((smp.shape[1], smp.shape[0]), np.inf)
    mu = x.sum(axis=2, keepdims=True) / k
    var = ((x - mu) ** 2).sum(axis=2) / (k - 1)
    var[(x == x[:, :, :1]).all(axis=2)] = 0.0  # equal samples: the rounding of sum / k is not variance
    return to_image(np.sqrt(var / k)).max(axis=2)


def largest_sample(smp, k):
    """per pixel the largest |sample| of the first k over the three channels; [row, column]"""
    return to_image(np.abs(smp[:, :, :k].astype(np.float64)).max(axis=2)).max(axis=2)


# ---- the quantiser -------------------------------------------------------------------------------------------------------------------------
def quantise(m):
    """core.clj:54-56 in float64: q = sqrt(m) * 255.99; NaN -> 0; else (int (min 255.99 q)), truncating"""
    m = np.asarray(m, np.float64)
    with np.errstate(invalid="ignore"):
        q = np.sqrt(m) * 255.99
    nan = np.isnan(q)
    return np.where(nan, 0.0, np.trunc(np.minimum(np.where(nan, 0.0, q), 255.99))).astype(np.uint8)


def bucket_borders():
    """for every k in 1..255 the smallest double whose quantised value is k, found by bisection over the bit patterns (the quantiser is
    monotone on [0, inf) and positive doubles order like their bit patterns); -> float64 [255]"""
    ks = np.arange(1, 256)
    lo = np.zeros(255, np.int64)                                    # quantise(0.0) = 0 < k
    hi = np.full(255, np.float64(2.0).view(np.int64), np.int64)     # quantise(2.0) = 255 >= k
    while (hi - lo > 1).any():
        mid = lo + (hi - lo) // 2
        up = quantise(mid.view(np.float64)) >= ks
        hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
    m = hi.view(np.float64)
    assert (quantise(m) == ks).all() and (quantise(np.nextafter(m, 0.0)) == ks - 1).all()
    return m


def around(m, n=2):
    """m, its n neighbours below and n above"""
    m = np.asarray(m, np.float64).ravel()
    out, lo, hi = [m], m, m
    for _ in range(n):
        lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
        out += [lo, hi]
    return np.concatenate(out)


def chosen_means():
    """bucket borders with their neighbours, the edges of the domain, values above 1, and what the quantiser's NaN branch is for"""
    tiny = np.float64(5e-324)
    special = np.array([0.0, -0.0, tiny, 2 * tiny, -tiny, 2.2250738585072014e-308, 1.5, 15.0, 1e300, 1.7976931348623157e308, np.inf, -np.inf,
                        -1.0, -1e-300, -0.25, -1e300, np.nan, -np.nan, 0.25, 0.5])
    return np.concatenate([around(bucket_borders()), around([1.0]), special])


# ---- the tile dealing of rtmi_assemble_device (include/rtmi.h), restated --------------------------------------------------------------------------
def tiles_of(nx, ny):
    return (nx + 7) // 8, (ny + 7) // 8


def deal(frame, world, per, poison=np.nan):
    """row-major frame [ny, nx, 3] -> gathered[world][per][64][3]: global tile g (row-major over the 8 x 8 tiles) is rank g % world's tile number
    g // world, pixel (x % 8, y % 8) of a tile is its element (y % 8) * 8 + x % 8.  Everything the frame does not cover -- padding slots, the
    out-of-frame pixels of edge tiles -- holds `poison`."""
    ny, nx, _ = frame.shape
    tx, ty = tiles_of(nx, ny)
    assert world * per >= tx * ty
    g = np.full((world, per, 64, 3), poison, np.float64)
    for y in range(ny):
        for x in range(nx):
            t = (y // 8) * tx + x // 8
            g[t % world, t // world, (y % 8) * 8 + x % 8] = frame[y, x]
    return g


def coded_tiles(nx, ny, world, per):
    """-> (gathered, frame): every in-frame element of every tile slot holds a value in (0, 1) that encodes (global tile, pixel in tile, channel),
    all different; written from the tile side, the frame it must assemble to from the pixel side"""
    tx, ty = tiles_of(nx, ny)
    n = tx * ty * 192

    def code(tile, pixel, channel):
        return ((tile * 64 + pixel) * 3 + channel + 0.5) / n

    g = np.full((world, per, 64, 3), np.nan)
    for t in range(tx * ty):
        for l in range(64):
            if (t % tx) * 8 + l % 8 < nx and (t // tx) * 8 + l // 8 < ny:
                g[t % world, t // world, l] = [code(t, l, c) for c in range(3)]
    yy, xx, cc = np.meshgrid(np.arange(ny), np.arange(nx), np.arange(3), indexing="ij")
    frame = code((yy // 8) * tx + xx // 8, (yy % 8) * 8 + xx % 8, cc)
    return g, np.ascontiguousarray(frame, np.float64)
