"""Shared by test_rays_reference.py (CPU) and test_gpu_rays.py (GPU): numpy restatements of what rtmi_render_rays does behind its paths -- the fold
of a group's rays, the group record that carries it over calls, the derived keys -- and the ray sets the two modules use.  Nothing here imports the
device library; the oracle is passed in.  Not a test module (pytest collects test_*.py only)."""
import numpy as np

import depth_cases as dc
import frame_reference as fr
import raytrace_clj_amd as r
from raytrace_clj_amd import flatten as fl

RAYS_REC = 10   # RTMI_RAYS_REC: sums rgb (in R, widened), Welford mean rgb, Welford M2 rgb, count
SEED = fr.SEED


def new_state(n_groups):
    return np.zeros((n_groups, RAYS_REC), np.float64)


def fold(rgb, group, precision="f64", first=0, state=None):
    """The radiance of n_groups * group rays [n, 3] (doubles holding values of R) -> (mean [n_groups, 3], stderr [n_groups]) over the rays
    [0, first + group) of every group; `state` ([n_groups, RAYS_REC], updated in place) carries rays [0, first) and must hold exactly them.
    Without a state `first` is not read.  include/rtmi.h restated:
      the sum in R, in row order, starting FROM the first ray; mean = sum * (R(1) / R(count)), widened;
      Welford in double: d = x - mu; mu += d / k; M2 += d * (x - mu) for the k-th ray (k >= 2); the first ray sets mu = x, M2 = 0;
      stderr = the largest channel's sqrt((M2 / (count - 1)) / count), a NaN never replacing the running maximum; +inf for count == 1."""
    R = fr.REAL[precision]
    rgb = np.asarray(rgb, np.float64).reshape(-1, group, 3)
    ng = len(rgb)
    if state is None:
        first = 0
    else:
        assert state.shape == (ng, RAYS_REC) and state.dtype == np.float64
    if first > 0:
        assert (state[:, 9] == first).all(), "a record continues with the count it holds"
        acc, mu, m2 = state[:, 0:3].astype(R), state[:, 3:6].copy(), state[:, 6:9].copy()
        assert np.array_equal(acc.astype(np.float64), state[:, 0:3])
    else:
        acc, mu, m2 = np.zeros((ng, 3), R), np.zeros((ng, 3)), np.zeros((ng, 3))
    with np.errstate(all="ignore"):
        for s in range(group):
            v = rgb[:, s].astype(R)
            if first + s == 0:
                acc, mu, m2 = v.copy(), v.astype(np.float64), np.zeros((ng, 3))
            else:
                acc = acc + v
                assert acc.dtype == R
                x = v.astype(np.float64)
                d = x - mu
                mu = mu + d / np.float64(first + s + 1)
                m2 = m2 + d * (x - mu)
        count = first + group
        if state is not None:
            state[:, 0:3], state[:, 3:6], state[:, 6:9], state[:, 9] = acc.astype(np.float64), mu, m2, count
        mean = (acc * (R(1.0) / R(count))).astype(np.float64)
        if count == 1:
            return mean, np.full(ng, np.inf)
        err = np.zeros(ng)
        for c in range(3):
            e = np.sqrt((m2[:, c] / np.float64(count - 1)) / np.float64(count))
            err = np.where(e > err, e, err)
    return mean, err


def derived_keys(seed, n_groups, group, g_first=0):
    """keys[g * group + r] = sample_key(seed, g, g_first + r): what the library derives when it is given no keys"""
    g, rr = (a.ravel() for a in np.meshgrid(np.arange(n_groups), np.arange(group), indexing="ij"))
    return fr.sample_keys(seed, g, g_first + rr)


# ---- ray sets ----------------------------------------------------------------------------------------------------------------------------------
SCENES = ("cover", "cornell", "hitlist-media")   # a sphere world, the Cornell box (mixed kinds), a world with media: names of depth_cases.SCENES
FRAME = (24, 16, 6)                              # the frame rendered through the front door


def pixel_major(per_sample, nx, ny, ns):
    """a per-sample array in depth_cases.frame_paths' [i, j, s] order -> the same rows grouped per pixel in IMAGE order (row 0 = top), samples in
    order: group y * nx + x holds pixel (i = x, j = ny - 1 - y)"""
    a = np.asarray(per_sample).reshape((nx, ny, ns) + np.asarray(per_sample).shape[1:])
    a = np.swapaxes(a, 0, 1)[::-1]               # [row, column, s, ...]
    return np.ascontiguousarray(a).reshape((nx * ny * ns,) + a.shape[3:])


_glass = {}


def glass_flat():
    """the glass-heavy world: the cover scene with choose-mat's thresholds at (0.1, 0.2) -- four of five small spheres are glass"""
    if "flat" not in _glass:
        _glass["flat"] = fl.flatten(r.scene.make_random_scene(64, 32, 11, False, mix=(0.1, 0.2)))
    return _glass["flat"]


N_GLASS = 2048


def refill_base(oracle):
    """2 * N_GLASS rays and keys: camera rays of the glass-heavy world, aimed below the horizon of the image (v < 1/2: the ground and the small
    spheres), interleaved one for one with rays that miss everything -- they start outside the sky dome and point away from it.  -> (rays, keys, ctr0)"""
    if "base" not in _glass:
        rng = np.random.default_rng(5)
        keys = rng.integers(0, 2 ** 63, 2 * N_GLASS, dtype=np.uint64)
        uv = rng.random((N_GLASS, 2)) * np.array([1.0, 0.5])
        cam = oracle.probe_camera(glass_flat(), uv, keys[0::2])
        rays = np.zeros((2 * N_GLASS, 7))
        rays[0::2] = cam[:, :7]
        rays[1::2] = np.array([0.0, 5000.0, 0.0, 0.0, 1.0, 0.0, 0.0]) + np.concatenate([rng.normal(size=(N_GLASS, 6)), np.zeros((N_GLASS, 1))], 1) * 0.1
        _glass["base"] = (rays, keys, int(cam[:, 7].max()))
    return _glass["base"]


def refill_set(oracle, n):
    """the base set repeated to at least n rays (a multiple of the base): every repetition traces the same paths"""
    rays, keys, ctr0 = refill_base(oracle)
    reps = -(-n // len(rays))
    return np.tile(rays, (reps, 1)), np.tile(keys, reps), ctr0


_pinhole = {}


def pinhole_flat(name):
    """a depth_cases scene behind a pinhole camera with the same image plane (every scene of the package has a thin lens, whose rays start their
    streams at different draws): a copy of the flattened scene, the camera record cut to origin, lower-left corner, horizontal, vertical"""
    if name not in _pinhole:
        import copy
        f = copy.copy(dc.flat(name))
        cam = np.zeros(24)
        cam[:12] = np.asarray(f.cam, np.float64)[:12]
        f.cam_kind, f.cam = 0, cam
        _pinhole[name] = f
    return _pinhole[name]
