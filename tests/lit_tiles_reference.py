"""Shared by test_lit_tiles_host.py (CPU) and test_gpu_lit_tiles.py (GPU): THE TILE ORDER of rtmi_render_lit_tiles* and the rule of
rtmi_tiles_retire* (include/rtmi.h) restated with numpy.  Nothing here imports the device library.  Not a test module."""
import numpy as np

TILE = 8


def tiles_of(nx, ny):
    """(tiles per row, tile rows) of the frame"""
    return (nx + TILE - 1) // TILE, (ny + TILE - 1) // TILE


def all_tiles(nx, ny):
    tx, ty = tiles_of(nx, ny)
    return np.arange(tx * ty, dtype=np.int32)


def row_map(nx, ny, s_first, s_count, tiles):
    """Row r of a call over `tiles` -> (x, y, s, has): sample s = s_first + r % s_count of local pixel (r // s_count) % 64 of tile
    tiles[r // (64 * s_count)]; has is False where the entry lies outside [0, T) or the pixel outside the image (x, y, s are then 0)."""
    tiles = np.asarray(tiles, np.int64).reshape(-1)
    tx, ty = tiles_of(nx, ny)
    r = np.arange(len(tiles) * 64 * s_count, dtype=np.int64)
    t = tiles[r // (64 * s_count)]
    l = (r // s_count) % 64
    listed = (t >= 0) & (t < tx * ty)
    tt = np.where(listed, t, 0)
    x = (tt % tx) * TILE + l % TILE
    y = (tt // tx) * TILE + l // TILE
    has = listed & (x < nx) & (y < ny)
    s = s_first + r % s_count
    return np.where(has, x, 0), np.where(has, y, 0), np.where(has, s, 0), has


def frame_rows(nx, ny, s_first, s_count, tiles):
    """-> (has, the row of rtmi_render_lit(nx, ny, s_first, s_count) that holds the same (pixel, sample), for the rows that have one)"""
    x, y, s, has = row_map(nx, ny, s_first, s_count, tiles)
    return has, ((y * nx + x) * s_count + (s - s_first))[has]


def pixel_mask(nx, ny, tiles):
    """[ny, nx] bool: the pixels of the listed tiles"""
    tx, ty = tiles_of(nx, ny)
    on = np.zeros(tx * ty, bool)
    t = np.asarray(tiles, np.int64).reshape(-1)
    on[t[(t >= 0) & (t < tx * ty)]] = True
    return np.repeat(np.repeat(on.reshape(ty, tx), TILE, axis=0), TILE, axis=1)[:ny, :nx]


def retire(noise, eps, tiles):
    """the survivors of `tiles`, in order: a tile survives if any of its pixels inside the image fails noise <= eps (NaN and +inf fail)"""
    ny, nx = noise.shape
    tx, ty = tiles_of(nx, ny)
    out = []
    for t in np.asarray(tiles, np.int64).reshape(-1):
        y0, x0 = (t // tx) * TILE, (t % tx) * TILE
        with np.errstate(invalid="ignore"):
            passes = noise[y0:y0 + TILE, x0:x0 + TILE] <= eps
        if not passes.all():
            out.append(t)
    return np.array(out, np.int32)


# the synthetic maps of the retire tests: (nx, ny) -> [(name, noise [ny, nx], eps)]
RETIRE_SHAPES = ((13, 7), (21, 19))


def retire_maps(nx, ny):
    rng = np.random.default_rng(nx * 1000 + ny)
    tx, ty = tiles_of(nx, ny)
    base = rng.random((ny, nx))
    maps = [("uniform", base.copy(), 0.5)]
    ties = np.full((ny, nx), 0.25)  # every pixel exactly at eps: all retire; then one pixel per other tile one ulp above
    maps.append(("ties-all-pass", ties.copy(), 0.25))
    above = ties.copy()
    for t in range(0, tx * ty, 2):
        y, x = min((t // tx) * TILE + 3, ny - 1), min((t % tx) * TILE + 5, nx - 1)
        above[y, x] = np.nextafter(0.25, 1.0)
    maps.append(("ties-one-ulp", above, 0.25))
    for name, v in (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf)):
        m = np.full((ny, nx), 0.1)
        m[ny - 1, nx - 1] = v  # the last pixel of the image: the corner tile, partial on both edges
        m[0, 0] = v if name != "-inf" else 0.1
        maps.append((name, m, 0.2))
    allneg = np.full((ny, nx), -np.inf)
    maps.append(("all -inf", allneg, 0.0))
    return maps
