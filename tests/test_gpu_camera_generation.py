"""Camera-ray generation of the trace kernels (generate_camera_rays: the wave-wide routine of both stash refills, with the cooperative lens-disk
sampler, the per-tile pixel hash, div_const for the jittered pixel coordinates) against the CPU oracle, which runs the sequential semantics.

The criterion is the one test_gpu_parity.py applies to frames: both counters (ray segments, pixels) equal the oracle's and the linear frame lies
within RMS_TOL.  A lane whose stream position after generation is off by one draw walks another path from its first scatter on, so the segment
count of small frames is a sharp check of the draw counts.  Frames are small (the oracle renders each once, cached per module); the claim is forced
to 256 items = 4 chunks, so that 3 and 17 samples per pixel make claims straddle tiles."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import raytrace_clj_amd as r
from raytrace_clj_amd import core
from raytrace_clj_amd import flatten as fl
from raytrace_clj_amd.util import draw_bits, sample_key, vec3

from test_gpu_parity import RMS_TOL, rms

SEED = core.RENDER_SEED
_expected = {}


def _cover(nx, ny, n, moving, aperture=0.0):
    sc = r.scene.make_random_scene(nx, ny, n, moving)
    if aperture:
        aspect = float(nx) / float(ny)
        sc = {"camera": r.camera.thin_lens_camera(lookfrom=vec3(13, 2, 3), lookat=vec3(0, 0, 0), vup=vec3(0, 1, 0), vfov=20, aspect=aspect,
                                                  aperture=aperture, focus_dist=10.0, t0=0.0, t1=1.0), "world": sc["world"]}
    return fl.flatten(sc)


def _oracle_frame(orc, tag, f, nx, ny, ns, seed=SEED, region=None):
    k = (tag, nx, ny, ns, seed, region)
    if k not in _expected:
        _expected[k] = orc.render(f, nx, ny, ns, 50, seed, region=region, nthreads=16)
    return _expected[k]


def _check(tag, got, exp):
    (lin, _, cnt), (exp_lin, _, exp_cnt) = got, exp
    err = rms(lin, exp_lin)
    print("%s: segments %d (oracle %d), pixels %d (%d), frame rms %.3g" % (tag, int(cnt[0]), int(exp_cnt[0]), int(cnt[1]), int(exp_cnt[1]), err))
    assert np.array_equal(cnt, exp_cnt), "%s: total-rays / total-pixels %s, the oracle's %s" % (tag, cnt, exp_cnt)
    assert err <= RMS_TOL, "%s: frame rms %.3g" % (tag, err)


@pytest.fixture(autouse=True)
def claim_256(monkeypatch):
    monkeypatch.setenv("RTMI_QUEUE_BLOCK_RT", "256")


@pytest.mark.parametrize("nx,ny", [(40, 24), (37, 21)])  # 37x21: partial tiles on both edges -- generations with item-less helper lanes
@pytest.mark.parametrize("moving", [False, True])
def test_cover_frames(oracle, nx, ny, moving):
    f = _cover(nx, ny, 3, moving)
    ds = core.DeviceScene(f)
    for ns in (1, 3, 17):
        _check("cover n=3 %dx%d moving=%s ns=%d" % (nx, ny, moving, ns), ds.render(nx, ny, ns), _oracle_frame(oracle, ("cover3", moving, 0.0), f, nx, ny, ns))
    ds.close()


def test_region_render(oracle):
    nx, ny, ns, region = 37, 21, 3, (5, 3, 30, 19)  # cuts tiles on all four sides: helper lanes inside full tiles too
    f = _cover(nx, ny, 3, False)
    ds = core.DeviceScene(f)
    _check("region", ds.render(nx, ny, ns, region=region), _oracle_frame(oracle, ("cover3", False, 0.0), f, nx, ny, ns, region=region))
    ds.close()


@pytest.mark.parametrize("n", [3, 11])
def test_open_aperture_carries_the_disk_values_back(oracle, n):
    """aperture 0.5: the winning candidate's x, y travel back to its victim and the stash holds the origins (17 words)"""
    nx, ny = 37, 21
    f = _cover(nx, ny, n, True, aperture=0.5)
    ds = core.DeviceScene(f)
    for ns in (1, 3):
        _check("aperture 0.5 n=%d ns=%d" % (n, ns), ds.render(nx, ny, ns), _oracle_frame(oracle, ("cover", n, True, 0.5), f, nx, ny, ns))
    ds.close()


@pytest.mark.parametrize("moving", [False, True])
@pytest.mark.parametrize("lds_stash", ["1", "0"])
def test_cover11_time_sliced_kernel_both_stashes(oracle, monkeypatch, moving, lds_stash):
    """the cover scene proper (n = 11: a tree of more than 128 nodes) runs the time-sliced kernel, the one that keeps the per-tile invariants;
    its camera-ray stash in LDS and (RTMI_SPHERE_LDS_STASH=0) in registers"""
    monkeypatch.setenv("RTMI_SPHERE_LDS_STASH", lds_stash)
    nx, ny = 37, 21
    f = _cover(nx, ny, 11, moving)
    ds = core.DeviceScene(f)
    for ns in (3, 17):
        _check("cover n=11 moving=%s lds_stash=%s ns=%d" % (moving, lds_stash, ns), ds.render(nx, ny, ns), _oracle_frame(oracle, ("cover11", moving), f, nx, ny, ns))
    ds.close()


def test_f32(oracle_f32):
    nx, ny, ns = 37, 21, 3
    f = _cover(nx, ny, 3, True)
    ds = core.DeviceScene(f)
    got = ds.render(nx, ny, ns, precision="f32")
    ds.close()
    _check("f32", got, oracle_f32.render(f, nx, ny, ns, 50, SEED, nthreads=16))


def test_cornell_box_mixed_kind_kernels_share_the_refill(oracle):
    from oracle.tree import flatten_with_tree
    f = flatten_with_tree(r.scene.make_cornell_box(24, 24))
    exp = oracle.render(f, 24, 24, 3, 50, SEED, nthreads=16)
    ctx = core.Context(0)
    ds = core.DeviceScene(f, ctx=ctx)
    for accel in (1, 0):
        ctx.set_option("accel", accel)
        _check("cornell accel %d" % accel, ds.render(24, 24, 3), exp)
    ds.close()
    ctx.close()


def _disk_rounds(key):
    """rounds of rand-in-unit-disk (util.clj:32-41) of a sample's stream: draws 0, 1 are the jitter, round k takes draws 2 + 2k, 3 + 2k"""
    for k in range(64):
        x, y = ((draw_bits(key, 2 + 2 * k + c) >> 11) * 2.0 ** -52 - 1.0 for c in (0, 1))
        if not x * x + y * y >= 1.0:
            return k + 1
    raise AssertionError("no accepted candidate in 64 rounds")


def test_rejection_tails(oracle):
    """the draw position of lanes deep in the rejection tail: a 32x16 frame (8 tiles = 512 keys at 1 spp) of a seed whose keys include lanes that need
    1, 2, 4 and 6 or more disk rounds (found on the host), rendered at 1 spp and depth 50; beside the frame criterion, the tail lanes' own pixels"""
    nx, ny = 32, 16
    seed = rounds = None
    for cand in range(1, 200):
        rr = np.array([[_disk_rounds(sample_key(cand, (ny - 1 - y) * nx + x, 0)) for x in range(nx)] for y in range(ny)])
        if {1, 2, 4} <= set(rr.ravel()) and rr.max() >= 6 and (rr >= 4).sum() >= 5:
            seed, rounds = cand, rr
            break
    assert seed is not None
    tail = rounds >= 4
    print("seed %d: rounds histogram %s, %d lanes need 4 or more" % (seed, np.bincount(rounds.ravel()).tolist(), int(tail.sum())))
    for moving, aperture in ((False, 0.0), (True, 0.5)):
        f = _cover(nx, ny, 3, moving, aperture)
        exp = oracle.render(f, nx, ny, 1, 50, seed, nthreads=16)
        ds = core.DeviceScene(f)
        got = ds.render(nx, ny, 1, seed=seed)
        ds.close()
        _check("tails seed %d aperture %s" % (seed, aperture), got, exp)
        err = float(np.abs(got[0][tail] - exp[0][tail]).max())
        print("tail pixels: max |colour - oracle| %.3g" % err)
        assert err <= 1e-12, "a lane that needs >= 4 disk rounds left generation at another stream position (its pixel is off by %.3g)" % err
