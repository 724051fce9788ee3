"""Shared by test_multi_progressive_host.py (CPU) and test_gpu_multi_progressive.py (GPU): the progressive tile record and its assembly
(rtmi_render_adaptive_tiles_device, rtmi_assemble_progressive_device) restated with numpy from the text of include/rtmi.h, and the frames a run of
progressive / adaptive calls over an explicit list of chunk sizes must produce, derived from the oracle's individual samples through
frame_reference and adaptive_reference.  Nothing here imports the device library; the oracle is passed in.  Not a test module."""
import numpy as np

import adaptive_reference as ar
import frame_reference as fr

REC = 5                 # RTMI_PROG_REC: mean r, g, b, stderr, samples
SIZE = (37, 21)         # 5 x 3 tiles, a partial right column and a partial bottom row
CHUNKS = (1, 3, 4)      # the first call leaves one sample behind every pixel: +inf in the records
WORLDS = (1, 2, 3, 4, 8)


# ---- the dealing and the record, from the header ----------------------------------------------------------------------------------------------
def n_tiles(nx, ny):
    tx, ty = fr.tiles_of(nx, ny)
    return tx * ty


def local_tiles(nx, ny, first, stride):
    """global tile indices of the dealing (first, stride): first, first + stride, ... below the number of tiles"""
    out, g = [], first
    while g < n_tiles(nx, ny):
        out.append(g)
        g += stride
    return out


def per_rank(nx, ny, world):
    """tiles every rank's record is padded to: the smallest count with world * count >= tiles"""
    per = 0
    while world * per < n_tiles(nx, ny):
        per += 1
    return per


def tile_record(linear, stderr, samples, g):
    """[64, 5] of global tile g (row-major over the 8 x 8 tiles): pixel l = row * 8 + column of the tile holds mean r, g, b, the standard error
    and the sample count as a double; a pixel outside the image holds five zeros"""
    ny, nx = stderr.shape
    tx, _ = fr.tiles_of(nx, ny)
    rec = np.zeros((64, REC))
    for l in range(64):
        x, y = (g % tx) * 8 + l % 8, (g // tx) * 8 + l // 8
        if x < nx and y < ny:
            rec[l, :3], rec[l, 3], rec[l, 4] = linear[y, x], stderr[y, x], float(samples[y, x])
    return rec


def dealt_records(linear, stderr, samples, first, stride, slots=None):
    """d_tiles_rec of the dealing (first, stride): [slots, 64, 5], local tile k = global tile first + k * stride; slots beyond the local tiles
    (the padding of a gathered record) hold zeros"""
    ny, nx = stderr.shape
    tiles = local_tiles(nx, ny, first, stride)
    slots = len(tiles) if slots is None else slots
    assert slots >= len(tiles)
    out = np.zeros((slots, 64, REC))
    for k, g in enumerate(tiles):
        out[k] = tile_record(linear, stderr, samples, g)
    return out


def gathered_records(linear, stderr, samples, world):
    """d_gathered_rec: [world, per, 64, 5], rank r's record is the dealing (r, world) padded to per tiles"""
    ny, nx = stderr.shape
    per = per_rank(nx, ny, world)
    return np.stack([dealt_records(linear, stderr, samples, r, world, per) for r in range(world)])


def assemble(gathered, nx, ny):
    """rtmi_assemble_progressive_device from the pixel side: pixel (x, y) lies in global tile t = (y // 8) * tiles_x + x // 8, which is rank
    t % world's tile number t // world -> (linear [ny, nx, 3], rgb8, stderr [ny, nx], samples int32 [ny, nx])"""
    world = gathered.shape[0]
    tx, _ = fr.tiles_of(nx, ny)
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    t = (yy // 8) * tx + xx // 8
    p = gathered[t % world, t // world, (yy % 8) * 8 + xx % 8]
    linear = np.ascontiguousarray(p[..., :3])
    return linear, fr.quantise(linear), np.ascontiguousarray(p[..., 3]), p[..., 4].astype(np.int32)


# ---- the frames of a run over explicit chunk sizes ---------------------------------------------------------------------------------------------
def ks_of(chunks):
    """k after every call"""
    return [int(k) for k in np.cumsum(chunks)]


def schedule_chunks(stderr_of, nx, ny, chunks, eps, retire=True):
    """adaptive_reference.schedule for calls of the sizes `chunks` (it knows first / chunk / cap runs only): every call gives its samples to the
    tiles active when it starts, then -- with retire, at k >= 2 -- retires the tiles whose pixels all pass se <= eps (a NaN fails).  Unlike
    refine_adaptive the calls go on when no tile is active (k advances).  -> list of (k, n_t [tiles_y, tiles_x], active [tiles_y, tiles_x])"""
    tx, ty = fr.tiles_of(nx, ny)
    n_t, active, out = np.zeros((ty, tx), np.int64), np.ones((ty, tx), bool), []
    for k in ks_of(chunks):
        n_t[active] = k
        if retire and k >= 2:
            with np.errstate(invalid="ignore"):
                active = active & ~(ar.tile_max(stderr_of(k)) <= eps)
        out.append((k, n_t.copy(), active.copy()))
    return out


class Run:
    """the oracle's samples of a frame_reference scene at SIZE with Welford's state after every call of CHUNKS"""

    def __init__(self, oracle, name, size=SIZE, chunks=CHUNKS):
        self.nx, self.ny = size
        self.name, self.precision, self.chunks = name, oracle.precision, tuple(chunks)
        self.smp, self.nseg = ar.samples(oracle, name, self.nx, self.ny, ks_of(chunks)[-1])
        self.m2 = ar.welford_m2(self.smp, ks_of(chunks))

    def stderr_of(self, k):
        return ar.stderr_plane(self.m2[k], k)

    def choose_eps(self, call=1):
        """midway inside the gap of the sorted per-tile maxima after call number `call` (0-based) that retires the tiles nearest to half of them
        -> (eps, tiles that retire in that call)"""
        v = np.sort(ar.tile_max(self.stderr_of(ks_of(self.chunks)[call])).ravel())
        v = v[np.isfinite(v)]
        half = n_tiles(self.nx, self.ny) // 2
        for n in sorted(range(1, len(v)), key=lambda n: abs(n - half)):
            if v[n - 1] < v[n]:
                return float(0.5 * (v[n - 1] + v[n])), n
        raise AssertionError("the per-tile maxima are all equal")

    def schedule(self, eps, retire=True):
        return schedule_chunks(self.stderr_of, self.nx, self.ny, self.chunks, eps, retire)

    def expected(self, n_t):
        """what the calls return while the tiles hold n_t samples -> (linear, rgb8, stderr, samples int32, ray segments)"""
        n_px = ar.per_pixel(n_t, self.nx, self.ny)
        linear = ar.expected_frame(self.smp, n_px)
        stderr = ar.compose(lambda n: self.stderr_of(n), n_px)
        return linear, fr.quantise(linear), stderr, n_px.astype(np.int32), ar.expected_rays(self.nseg, n_px)
