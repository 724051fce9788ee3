"""Shared by test_lit_host.py (CPU) and test_gpu_lit.py (GPU): the frame rule of rtmi_render_lit restated from the pieces the suite already has --
depth_cases.frame_paths (every sample's camera ray, key and the draw its path starts at), rays_reference.pixel_major (the call's row order) and
rays_reference.fold.  Nothing here imports the device library; the probes are passed in.  Not a test module (pytest collects test_*.py only).

The call's rows: group g = y * nx + x is pixel (x, y), row 0 at the top; row g * ns + s is its sample s.  depth_cases.frame_paths numbers the samples
[i, j, s] with j = 0 at the bottom; pixel_major turns one order into the other."""
import numpy as np

import depth_cases as dc
import rays_reference as rr

SEED = dc.SEED
SHAPES = ((13, 7, 3), (40, 24, 2), rr.FRAME)  # 273 items: nx no multiple of 8, a last wave of 17 lanes; 30 full waves; the frame of the ray tests
SMALL = SHAPES[0]
ESTIMATORS = {"plain": 0, "nee": 1, "mis": 2}


def frame_groups(probe_camera, f, nx, ny, ns, seed=SEED, s_first=0):
    """-> (rays [n, 7], keys [n], ctr [n]) of samples [s_first, s_first + ns) of every pixel in the call's row order (aperture-0 cameras, FP64:
    depth_cases.frame_paths' conditions).  probe_camera(uv, keys) -> [n, 8] is the oracle's or the device's."""
    rays, keys, ctr = dc.frame_paths(probe_camera, f, nx, ny, s_first + ns, seed)
    cut = lambda a: rr.pixel_major(a, nx, ny, s_first + ns).reshape((nx * ny, s_first + ns) + a.shape[1:])[:, s_first:]
    rays, keys, ctr = cut(rays), cut(keys), cut(ctr)
    return np.ascontiguousarray(rays).reshape(-1, 7), np.ascontiguousarray(keys).ravel(), np.ascontiguousarray(ctr).ravel()


def frame_keys(nx, ny, ns, seed=SEED, s_first=0):
    """the keys of the frame rule's step 2 in the call's row order: sample_key(seed, j * nx + x, s), j = ny - 1 - y"""
    import frame_reference as fr
    y, x, s = (a.ravel() for a in np.meshgrid(np.arange(ny), np.arange(nx), np.arange(s_first, s_first + ns), indexing="ij"))
    return fr.sample_keys(seed, (ny - 1 - y) * nx + x, s)


def probe_by_ctr(probe, rays, keys, ctr, **kw):
    """probe(rays, keys, ctr0=, **kw) -> a tuple of per-path arrays (or None), for paths that start at different draws: one call per distinct ctr,
    the rows put back in order"""
    ctr = np.asarray(ctr).astype(np.int64)
    out = None
    for c in np.unique(ctr):
        pick = np.flatnonzero(ctr == c)
        part = probe(rays[pick], keys[pick], ctr0=int(c), **kw)
        if out is None:
            out = [None if p is None else np.zeros((len(keys),) + p.shape[1:], p.dtype) for p in part]
        for o, p in zip(out, part):
            if o is not None:
                o[pick] = p
    return tuple(out)


def folded_frame(rgb, nx, ny, ns, precision="f64"):
    """per-row radiance in the call's order -> (linear [ny, nx, 3], stderr [ny, nx]): rays_reference.fold per pixel"""
    mean, err = rr.fold(rgb, ns, precision)
    return mean.reshape(ny, nx, 3), err.reshape(ny, nx)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)
