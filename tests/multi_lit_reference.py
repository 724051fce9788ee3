"""Shared by test_multi_lit_host.py (CPU) and test_gpu_multi_lit.py (GPU): THE DEALT LIT FRAME of include/rtmi.h restated with numpy from the header's
text -- the dealing, the padding, the record rtmi_lit_tiles_records_device packs out of a replica's whole-frame buffers, the assembly of the gathered
records, the retirement of a list by a map and the merge of the replicas' lists.  Nothing here imports the device library.  Not a test module."""
import numpy as np

REC = 5          # RTMI_PROG_REC: mean r, g, b, stderr, samples
RAYS_REC = 10    # RTMI_RAYS_REC: word [9] of a pixel's state record is its sample count
TILE = 8
MAX_REPLICAS = 8  # RTMI_MULTI_LIT_MAX
SIZE = (37, 21)  # 5 x 3 tiles, a partial right column and a partial bottom row
SMALL = (9, 9)   # 4 tiles: with 8 replicas four of them own none
CHUNKS = (1, 3, 4)
WORLDS = (1, 2, 3, 8)


def tiles_xy(nx, ny):
    return -(-nx // TILE), -(-ny // TILE)


def n_tiles(nx, ny):
    tx, ty = tiles_xy(nx, ny)
    return tx * ty


def owned(nx, ny, r, n):
    """the dealing: replica r of n owns tiles r, r + n, ... below T, ascending (none when r >= T)"""
    return [t for t in range(n_tiles(nx, ny)) if t % n == r]


def per_replica(nx, ny, n):
    """slots of every replica's record: ceil(T / n)"""
    return -(-n_tiles(nx, ny) // n)


def record_words(nx, ny, n):
    """eight-byte words one gather moves per replica: the tiles, then the call's four counters"""
    return per_replica(nx, ny, n) * 64 * REC + 4


def records(state, linear, stderr, nx, ny, tile_first, tile_stride, n_slots):
    """rtmi_lit_tiles_records_device: [n_slots, 64, 5]; slot k is global tile tile_first + k * tile_stride, local pixel l = row * 8 + column.  The mean and
    the error are the planes' values as they are, the samples word [9] of the pixel's state record; a pixel outside the image and every pixel of a slot
    whose tile is at or past T hold five zeros."""
    tx, _ = tiles_xy(nx, ny)
    state = np.asarray(state).reshape(ny, nx, RAYS_REC)
    out = np.zeros((n_slots, 64, REC))
    for k in range(n_slots):
        g = tile_first + k * tile_stride
        if g >= n_tiles(nx, ny):
            continue
        for l in range(64):
            x, y = (g % tx) * TILE + l % TILE, (g // tx) * TILE + l // TILE
            if x < nx and y < ny:
                out[k, l, :3], out[k, l, 3], out[k, l, 4] = linear[y, x], stderr[y, x], state[y, x, 9]
    return out


def gathered(state, linear, stderr, nx, ny, n):
    """[n, per, 64, 5]: replica r's record is the dealing (r, n) padded to per slots"""
    return np.stack([records(state, linear, stderr, nx, ny, r, n, per_replica(nx, ny, n)) for r in range(n)])


def quantise(linear):
    """sqrt, x 255.99, min, truncation, NaN -> 0 on the double mean"""
    with np.errstate(invalid="ignore"):
        q = np.sqrt(np.asarray(linear, np.float64)) * 255.99
    q = np.where(q < 255.99, q, 255.99)
    return np.where(np.isnan(q), 0.0, q).astype(np.int64).astype(np.uint8)


def assemble(g, nx, ny):
    """the gathered records from the pixel side: pixel (x, y) lies in global tile t, which is replica t % n's slot t // n
    -> (linear [ny, nx, 3], rgb8, stderr [ny, nx], samples int32 [ny, nx])"""
    n = g.shape[0]
    tx, _ = tiles_xy(nx, ny)
    yy, xx = np.meshgrid(np.arange(ny), np.arange(nx), indexing="ij")
    t = (yy // TILE) * tx + xx // TILE
    p = g[t % n, t // n, (yy % TILE) * TILE + xx % TILE]
    linear = np.ascontiguousarray(p[..., :3])
    return linear, quantise(linear), np.ascontiguousarray(p[..., 3]), p[..., 4].astype(np.int32)


def survivors(noise, eps, tiles, nx, ny):
    """rtmi_tiles_retire's rule: a listed tile survives if any of its pixels inside the image fails noise <= eps (a NaN fails)"""
    tx, _ = tiles_xy(nx, ny)
    keep = []
    for t in tiles:
        x0, y0 = (t % tx) * TILE, (t // tx) * TILE
        with np.errstate(invalid="ignore"):
            if not (noise[y0:min(y0 + TILE, ny), x0:min(x0 + TILE, nx)] <= eps).all():
                keep.append(int(t))
    return keep


def merged(lists):
    """rtmi_multi_lit_active_tiles: the replicas' lists in ascending order"""
    return np.array(sorted(t for one in lists for t in one), np.int32)
