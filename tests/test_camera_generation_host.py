"""Host-side pins of the wave-wide camera-ray generation (no device): the correctly rounded quotient by a launch constant that replaces the two
divisions of start_sample in the FP64 kernels, and the certificates that let the refill skip the lens offset (scene_build.h)."""
import ctypes
import ctypes.util

import numpy as np

import raytrace_clj_amd as r
from raytrace_clj_amd import _ffi
from raytrace_clj_amd import flatten as fl
from raytrace_clj_amd.util import vec3


def test_div_const_is_the_ieee_quotient_of_pixel_coordinates():
    """div_const(x, n, RN(1/n)) = fma(fma(-n, q, x), rn, q) with q = RN(x rn) against x / n: x = i + u on the 2^-53 grid of a draw, 0 <= x <= n,
    for every n up to 512 (powers of two and not), frame widths in use and the largest int"""
    libm = ctypes.CDLL(ctypes.util.find_library("m"))
    libm.fma.restype = ctypes.c_double
    libm.fma.argtypes = [ctypes.c_double] * 3
    fma = libm.fma
    rng = np.random.default_rng(5)
    checked = 0
    for n in list(range(1, 513)) + [1080, 1920, 2160, 3840, 4320, 7680, 65535, 65536, 1000003, 16777216, 2 ** 31 - 1]:
        c, rn = float(n), 1.0 / float(n)
        i = rng.integers(0, n, 60).astype(np.float32).astype(np.float64)  # (R)(float)i of start_sample
        u = rng.integers(0, 2 ** 53, 60).astype(np.float64) * 2.0 ** -53
        xs = np.concatenate([i + u, [0.0, 2.0 ** -53, float(n - 1), float(n - 1) + (1.0 - 2.0 ** -53), float(n)]])
        for x in xs:
            x = float(x)
            q = x * rn
            assert fma(fma(-c, q, x), rn, q) == x / c, (n, x)
            checked += 1
    assert checked > 30000


def _flags(cam_kind, cam):
    cam = np.ascontiguousarray(cam, np.float64)
    return int(_ffi.lib().rtmi_test_camera_fixed(int(cam_kind), _ffi.ptr(cam)))


def test_fixed_ray_certificates():
    f = fl.flatten(r.scene.make_random_scene(40, 24, 3, False))
    cam, kind = np.array(f.cam, np.float64), int(f.cam_kind)
    assert kind == fl.CAM_THINLENS and cam[21] == 0.0
    assert _flags(kind, cam) == 3, "the cover scene: aperture 0 -- fixed origin and fixed direction"
    open_lens = cam.copy(); open_lens[21] = 0.5
    assert _flags(kind, open_lens) == 0
    assert _flags(fl.CAM_PINHOLE, cam) == 1, "a pinhole camera draws no lens disk: fixed origin only"
    for k in (3, 4, 5):  # a lower-left corner component that is -0, in double or only as a float: the direction is not certified, the origin still is
        for v in (-0.0, -1e-60):
            c = cam.copy(); c[k] = v
            assert _flags(kind, c) == 1, (k, v)
        c = cam.copy(); c[k] = 0.0
        assert _flags(kind, c) == 3
    for k in (0, 1, 2):  # the same in the origin: neither certificate
        for v in (-0.0, -1e-60, np.inf):
            c = cam.copy(); c[k] = v
            assert _flags(kind, c) == 0, (k, v)
    c = cam.copy(); c[12] = np.nan
    assert _flags(kind, c) == 0
