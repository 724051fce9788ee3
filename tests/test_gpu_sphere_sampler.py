"""The cooperative round of rand_in_unit_sphere_wave (rtmi_device.h) with its lane split taken from kCoopSplit: exact victim counts through
DeviceScene.probe_scatter, and frames in which idle, parked and dead lanes are the helpers.

probe_scatter gives every thread one material, so every lane of a full wave needs a sample and the number of lanes still pending after the
plain rounds -- the n of the first cooperative round, which decides K = 64 / n and the lane -> (candidate, victim) map -- follows from the keys
alone.  The batches are built for one, two and three plain candidates, so that each n is met whichever schedule the library is built with.  The host classifies keys by the index of their first accepted candidate (candidate c is draws 3c, 3c+1, 3c+2 of the stream, accepted if
not x^2 + y^2 + z^2 >= 1: util.clj:43-52) and builds waves with a chosen n.  The result must be the oracle's sequential loop bit for bit, the
draw count (column 8) included.

The frames use the criterion of test_gpu_camera_generation.py: both counters equal the oracle's and the frame within RMS_TOL (a lane that leaves
the sampler one draw off walks another path from there on, so the segment count of a small frame is a sharp check).  They render the scenes
of that file's cover-11, Cornell-box and FP32 tests, but without its RTMI_QUEUE_BLOCK_RT=256 fixture: the library's own claim size, so other
lanes of a wave are parked or dead when the sampler runs.  The oracle's frames are shared with that file (one cache).  What pins the round
itself are the probe_scatter tests: an independent oracle, n chosen on the host, draw counts asserted."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raytrace_clj_amd as r
from raytrace_clj_amd import core
from raytrace_clj_amd import flatten as fl
from raytrace_clj_amd.util import draw_bits, vec3

from test_gpu_camera_generation import SEED, _check, _cover, _oracle_frame

PLAIN = (1, 2, 3)  # candidates a lane tries on its own before the wave helps: the values RTMI_SAMPLER_PLAIN can be built with; batches are made for each
DEEP = 8  # 3 plain candidates + the K = 5 of a first round with n = 12: a victim whose first acceptance is here or later meets a second round
VICTIMS = [1, 2, 3, 5, 7, 12, 13, 21, 31, 32, 33, 63, 64]  # remainders of 64 / n, K = 1 above 32, every lane a victim
KEY_POOL = range(1, 6000)


def _first_accepted(key):
    """index of the first accepted candidate of rand-in-unit-sphere on the stream of `key` from draw 0"""
    for c in range(64):
        x, y, z = ((draw_bits(key, 3 * c + k) >> 11) * 2.0 ** -52 - 1.0 for k in range(3))
        if not (x * x + y * y) + z * z >= 1.0:
            return c
    raise AssertionError("no accepted candidate in 64")


@pytest.fixture(scope="module")
def classified():
    first = {k: _first_accepted(k) for k in KEY_POOL}
    pools = {}
    for plain in PLAIN:
        quick = [k for k in KEY_POOL if first[k] < plain]
        slow = [k for k in KEY_POOL if first[k] >= plain]
        deep = [k for k in slow if first[k] >= DEEP]
        print("keys 1..%d: %d pending after %d candidates, %d with the first acceptance at index >= %d" % (KEY_POOL[-1], len(slow), plain, len(deep), DEEP))
        assert len(slow) >= 64 + 17 and len(quick) >= 64 and deep
        pools[plain] = (quick, slow, deep)
    return first, pools


def _wave(classified, n, salt, want_deep=False, plain=PLAIN[0]):
    """64 keys of which exactly n are pending after `plain` candidates, scattered over the lanes"""
    first, (quick, slow, deep) = classified[0], classified[1][plain]
    rng = np.random.default_rng(1000 * n + salt)
    pend = [int(k) for k in rng.choice([k for k in slow if k not in deep] if want_deep else slow, n - (1 if want_deep else 0), replace=False)]
    if want_deep:
        pend.append(deep[salt % len(deep)])
    keys = pend + [int(k) for k in rng.choice(quick, 64 - n, replace=False)]
    keys = [keys[i] for i in rng.permutation(64)]
    assert sum(first[k] >= plain for k in keys) == n
    return keys


@pytest.fixture(scope="module")
def scatter_scene(oracle):
    mats = [r.shader.lambertian(albedo=r.texture.constant(color=vec3(0.4, 0.2, 0.1))),
            r.shader.metal(albedo=r.texture.constant(color=vec3(0.7, 0.6, 0.5)), fuzz=0.7)]
    world = r.hitable.hitlist(items=[r.hitable.sphere(center=vec3(3 * k, 0, 0), radius=1.0, material=m) for k, m in enumerate(mats)])
    f = fl.flatten(world, r.camera.PinholeCamera(*(np.zeros(3),) * 4))
    ds = core.DeviceScene(f)
    yield f, ds
    ds.close()


def _records(n, seed):
    rng = np.random.default_rng(seed)
    nrm = rng.normal(size=(n, 3)); nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    rays = np.concatenate([rng.normal(size=(n, 3)), rng.normal(size=(n, 3)) * 3, rng.random((n, 1))], axis=1)
    hits = np.concatenate([rng.normal(size=(n, 3)), nrm, rng.random((n, 2))], axis=1)
    return rays, hits


def _compare(oracle, scatter_scene, first, keys, tag):
    f, ds = scatter_scene
    keys = np.array(keys, np.uint64)
    rays, hits = _records(len(keys), 7)
    for mat in (0, 1):  # Lambertian, Metal with fuzz 0.7
        got, exp = ds.probe_scatter(mat, rays, hits, keys), oracle.probe_scatter(f, mat, rays, hits, keys)
        assert np.array_equal(exp[:, 8], [3.0 * (first[int(k)] + 1) for k in keys]), "%s: the host's classification is not the oracle's loop" % tag
        bad = np.flatnonzero(~(got == exp).all(axis=1))
        assert np.array_equal(got, exp), "%s material %d: lanes %s differ; draws %s, the oracle's %s" % (tag, mat, bad.tolist(), got[bad, 8].tolist(), exp[bad, 8].tolist())


@pytest.mark.parametrize("n", VICTIMS)
def test_exact_victim_counts(oracle, scatter_scene, classified, n):
    first = classified[0]
    for plain in PLAIN:
        for salt in (0, 1):
            keys = _wave(classified, n, salt, want_deep=(n == 12), plain=plain)
            if n == 12:  # past the plain candidates and the K = 5 of the first cooperative round: this victim advances by 3 K and meets a second round
                assert max(first[k] for k in keys) >= DEEP
            _compare(oracle, scatter_scene, first, keys, "n=%d plain=%d salt=%d" % (n, plain, salt))


def test_several_waves_and_a_partial_last_wave(oracle, scatter_scene, classified):
    """64 + 17 threads: the second wave is partial (its other lanes have left the kernel) and takes the plain loop; every one of its lanes pending"""
    first, (quick, slow, deep) = classified[0], classified[1][PLAIN[0]]
    keys = _wave(classified, 21, 5) + slow[:16] + [deep[0]]
    _compare(oracle, scatter_scene, first, keys, "64 + 17")


@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("lds_stash", ["1", "0"])
def test_cover11_frames_parked_and_dead_lanes_help(oracle, monkeypatch, moving, lds_stash):
    """scene n = 11 at 37x21 (partial tiles: item-less lanes) runs the time-sliced kernel: parked and dead lanes of the wave are helpers"""
    monkeypatch.setenv("RTMI_SPHERE_LDS_STASH", lds_stash)
    nx, ny = 37, 21
    f = _cover(nx, ny, 11, moving)
    ds = core.DeviceScene(f)
    for ns in (3, 17):
        _check("sampler cover n=11 moving=%s lds_stash=%s ns=%d" % (moving, lds_stash, ns), ds.render(nx, ny, ns), _oracle_frame(oracle, ("cover11", moving), f, nx, ny, ns))
    ds.close()


def test_cornell_box_both_accels(oracle):
    """the mixed-kind kernels"""
    from oracle.tree import flatten_with_tree
    f = flatten_with_tree(r.scene.make_cornell_box(24, 24))
    exp = _oracle_frame(oracle, ("cornell-tree",), f, 24, 24, 3)
    ctx = core.Context(0)
    ds = core.DeviceScene(f, ctx=ctx)
    for accel in (1, 0):
        ctx.set_option("accel", accel)
        _check("sampler cornell accel %d" % accel, ds.render(24, 24, 3), exp)
    ds.close()
    ctx.close()


def test_f32_frame(oracle_f32):
    nx, ny, ns = 37, 21, 3
    f = _cover(nx, ny, 3, True)
    ds = core.DeviceScene(f)
    got = ds.render(nx, ny, ns, precision="f32")
    ds.close()
    _check("sampler f32", got, oracle_f32.render(f, nx, ny, ns, 50, SEED, nthreads=16))
