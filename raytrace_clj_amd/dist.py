"""One process per GPU: the framebuffer is cut into 8x8 tiles dealt round-robin to ranks (the reference's
tiled-coords chunks, core.clj:59-71, become device tiles), every rank renders its tiles from a replicated scene,
and ONE gather (RCCL over xGMI when the backend is nccl) brings the tile-major buffers to rank 0, which un-tiles and
quantises them on its GPU.  Pixels are independent and the stream key is the global pixel index, so the image does not
depend on the partition."""
import ctypes as C

import numpy as np
import torch
import torch.distributed as dist

from . import _ffi
from . import core
from . import flatten as fl
from .core import Context, DeviceScene, check

TILE = _ffi.TILE
HOST_STAGED_GATHER = False  # rehearsal only (gloo on a one-GPU box): stage the gather through host memory


def n_tiles(nx, ny):
    return ((nx + TILE - 1) // TILE) * ((ny + TILE - 1) // TILE)


def tiles_per_rank(nx, ny, world):
    """every rank's buffer is padded to this many tiles so the gather is uniform"""
    return (n_tiles(nx, ny) + world - 1) // world


def local_tile_ids(nx, ny, rank, world):
    """global tile indices rank `rank` renders: rank, rank + world, ..."""
    return list(range(rank, n_tiles(nx, ny), world))


def gather_tiles(local_tiles, world, rank, dst=0, group=None):
    """local_tiles: [tiles_per_rank, 64, 3] float64 on this rank's device -> on dst: [world, tiles_per_rank, 64, 3]
    (any trailing shape: the progressive tile records are [tiles_per_rank, 64, 5])."""
    if world == 1:
        return local_tiles.unsqueeze(0)
    if HOST_STAGED_GATHER:
        host = local_tiles.cpu()
        if rank == dst:
            out = torch.empty((world,) + tuple(host.shape), dtype=host.dtype)
            dist.gather(host, list(out.unbind(0)), dst=dst, group=group)
            return out.to(local_tiles.device)
        dist.gather(host, None, dst=dst, group=group)
        return None
    if rank == dst:
        out = torch.empty((world,) + tuple(local_tiles.shape), dtype=local_tiles.dtype, device=local_tiles.device)
        dist.gather(local_tiles, list(out.unbind(0)), dst=dst, group=group)
        return out
    dist.gather(local_tiles, None, dst=dst, group=group)
    return None


class TileRenderer:
    """Per-rank driver of the tile-partitioned render."""

    def __init__(self, device_scene, nx, ny, rank, world):
        self.ds, self.nx, self.ny, self.rank, self.world = device_scene, nx, ny, rank, world
        self.per = tiles_per_rank(nx, ny, world)
        dev = torch.device("cuda", device_scene.ctx.device)
        self.dev, self._side, self._ev = dev, None, None
        self.local = torch.zeros((self.per, 64, 3), dtype=torch.float64, device=dev)
        self.counters = torch.zeros(2, dtype=torch.int64, device=dev)
        if rank == 0:
            self.linear = torch.zeros((ny, nx, 3), dtype=torch.float64, device=dev)
            self.rgb8 = torch.zeros((ny, nx, 3), dtype=torch.uint8, device=dev)

    def step(self, ns, depth=50, seed=0x5EED0002, precision="f64"):
        """render local tiles -> gather -> (rank 0) assemble.  Asynchronous, ordered with torch's current stream.

        The C-ABI reads stream handle 0 (NULL) as "the context's own stream", and torch's default stream has handle 0: on
        the default stream the render would run un-ordered with torch's work (the zero-fill of the buffers above, the
        gather).  So from the default stream the whole step runs on a side stream that first waits for the current stream
        and that the current stream then waits for."""
        cur = torch.cuda.current_stream(self.dev)
        if cur.cuda_stream != 0:
            return self._step(cur.cuda_stream, ns, depth, seed, precision)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.dev)
        self._side.wait_stream(cur)
        with torch.cuda.stream(self._side):
            self._step(self._side.cuda_stream, ns, depth, seed, precision)
        cur.wait_stream(self._side)

    def _step(self, stream, ns, depth, seed, precision):
        self.ds.render_tiles_device(self.nx, self.ny, ns, self.rank, self.world, self.local, self.counters, depth, seed, precision, stream)
        if self.world > 1:
            if self._ev is None:
                self._ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self._ev[0].record()
        gathered = gather_tiles(self.local, self.world, self.rank)
        if self.world > 1:
            self._ev[1].record()
        if self.rank == 0:
            check(_ffi.lib().rtmi_assemble_device(self.ds.ctx.handle, self.nx, self.ny, self.world, self.per, _ffi.ptr(gathered),
                                                  _ffi.ptr(self.linear), _ffi.ptr(self.rgb8), _ffi.ptr(stream)))

    def step_adaptive(self, s_first, s_count, retire, eps=0.0, depth=50, seed=0x5EED0002, precision="f64"):
        """One refinement of the frame dealt over the ranks: samples [s_first, s_first + s_count) into this rank's tiles (retire: the adaptive
        rule with eps, else none retires) -> gather of the tile records -> (rank 0) assemble into self.linear, self.rgb8, self.stderr,
        self.samples.  Ordered with torch's current stream as step() is; the render call synchronises its stream once (the host mirrors the
        rank's active list: self.ds.ctx.adaptive_status() / adaptive_active_tiles() describe this rank's tiles)."""
        if getattr(self, "local_rec", None) is None:
            self.local_rec = torch.zeros((self.per, 64, _ffi.PROG_REC), dtype=torch.float64, device=self.dev)
            if self.rank == 0:
                self.stderr = torch.zeros((self.ny, self.nx), dtype=torch.float64, device=self.dev)
                self.samples = torch.zeros((self.ny, self.nx), dtype=torch.int32, device=self.dev)
        cur = torch.cuda.current_stream(self.dev)
        if cur.cuda_stream != 0:
            return self._step_adaptive(cur.cuda_stream, s_first, s_count, retire, eps, depth, seed, precision)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.dev)
        self._side.wait_stream(cur)
        with torch.cuda.stream(self._side):
            self._step_adaptive(self._side.cuda_stream, s_first, s_count, retire, eps, depth, seed, precision)
        cur.wait_stream(self._side)

    def _step_adaptive(self, stream, s_first, s_count, retire, eps, depth, seed, precision):
        # (the primitive writes this rank's local tiles only: the padding slot of local_rec, if any, keeps its zeros)
        self.ds.render_adaptive_tiles_device(self.nx, self.ny, s_first, s_count, retire, eps, self.rank, self.world, self.local_rec, self.counters,
                                             depth, seed, precision, stream)
        gathered = gather_tiles(self.local_rec, self.world, self.rank)
        if self.rank == 0:
            self.ds.ctx.assemble_progressive_device(self.nx, self.ny, self.world, self.per, gathered, self.linear, self.rgb8, self.stderr,
                                                    self.samples, stream)

    def step_lit(self, s_first, s_count, estimator="mis", volume=False, lights=None, light_choice=0, depth=core.DEFAULT_DEPTH, seed=core.RENDER_SEED,
                 precision="f64"):
        """One refinement of the light-sampled frame dealt over the ranks (the one-process-per-GPU form of MultiDevice.lit_render): samples
        [s_first, s_first + s_count) into this rank's listed tiles (render_lit_tiles_device, or render_lit_ris_device for estimator "ris", on
        whole-frame buffers the rank holds) -> the records of its dealt tiles (lit_tiles_records_device) -> gather -> (rank 0) assemble into
        self.linear, self.rgb8, self.stderr, self.samples.  self.lit_counters holds the call's four counters of this rank.  The rank's list is
        self.lit_tiles[:self.lit_active], all its dealt tiles at first; retire_lit shortens it.  Ordered with torch's current stream as step() is."""
        if getattr(self, "lit_state", None) is None:
            f64 = dict(dtype=torch.float64, device=self.dev)
            own = local_tile_ids(self.nx, self.ny, self.rank, self.world)
            self.lit_state = torch.zeros((self.nx * self.ny, _ffi.RAYS_REC), **f64)
            self.lit_linear, self.lit_stderr = torch.zeros((self.ny, self.nx, 3), **f64), torch.zeros((self.ny, self.nx), **f64)
            self.lit_tiles = torch.tensor(own if own else [0], dtype=torch.int32, device=self.dev)
            self.lit_active = len(own)
            self.lit_counters = torch.zeros(4, dtype=torch.int64, device=self.dev)
            self.lit_rec = torch.zeros((self.per, 64, _ffi.PROG_REC), **f64)
            if self.rank == 0 and getattr(self, "stderr", None) is None:
                self.stderr = torch.zeros((self.ny, self.nx), **f64)
                self.samples = torch.zeros((self.ny, self.nx), dtype=torch.int32, device=self.dev)
        args = (s_first, s_count, estimator, volume, lights, light_choice, depth, seed, precision)
        cur = torch.cuda.current_stream(self.dev)
        if cur.cuda_stream != 0:
            return self._step_lit(cur.cuda_stream, *args)
        if self._side is None:
            self._side = torch.cuda.Stream(device=self.dev)
        self._side.wait_stream(cur)
        with torch.cuda.stream(self._side):
            self._step_lit(self._side.cuda_stream, *args)
        cur.wait_stream(self._side)

    def _step_lit(self, stream, s_first, s_count, estimator, volume, lights, light_choice, depth, seed, precision):
        kw = dict(lights=lights, depth=depth, seed=seed, precision=precision, state=self.lit_state, out_counters=self.lit_counters, stream=stream)
        if self.lit_active == 0:
            self.lit_counters.zero_()  # (a call without a tile traces nothing and writes no counter)
        if isinstance(estimator, str) and estimator == "ris":
            if volume:
                raise ValueError("estimator \"ris\" has no volume form")
            self.ds.render_lit_ris_device(self.nx, self.ny, s_first, s_count, self.lit_linear, self.lit_stderr, None, n_tiles=self.lit_active,
                                          tiles=self.lit_tiles, **kw)
        else:
            self.ds.render_lit_tiles_device(self.nx, self.ny, s_first, s_count, self.lit_active, self.lit_tiles, self.lit_linear, self.lit_stderr, None,
                                            estimator=estimator, volume=volume, light_choice=light_choice, **kw)
        self.ds.ctx.lit_tiles_records_device(self.nx, self.ny, self.rank, self.world, self.per, self.lit_state, self.lit_linear, self.lit_stderr,
                                             self.lit_rec, stream)
        gathered = gather_tiles(self.lit_rec, self.world, self.rank)
        if self.rank == 0:
            self.ds.ctx.assemble_progressive_device(self.nx, self.ny, self.world, self.per, gathered, self.linear, self.rgb8, self.stderr,
                                                    self.samples, stream)

    def retire_lit(self, eps, noise=None):
        """tiles_retire_device on this rank's list (noise None: the rank's own stderr plane, valid on exactly its own tiles; else a whole-frame
        [ny, nx] map on this rank's device) -> tiles still listed on this rank.  Synchronises the current stream once."""
        cur = torch.cuda.current_stream(self.dev)
        cur.synchronize()
        self.lit_active = self.ds.ctx.tiles_retire_device(self.nx, self.ny, self.lit_stderr if noise is None else noise, eps, self.lit_active,
                                                          self.lit_tiles)
        torch.cuda.synchronize(self.dev)
        return self.lit_active

    def last_gather_ms(self):
        """milliseconds the last step's gather took on this rank's stream (the transfer plus the wait for the slowest rank)"""
        if self._ev is None:
            return 0.0
        self._ev[1].synchronize()
        return self._ev[0].elapsed_time(self._ev[1])


class MultiDevice:
    """ONE host process driving several GPUs through the C-ABI (rtmi_render_multi*): what a one-JVM host of the reference
    (core.clj:100-108) calls.  devices = HIP device ordinals, one replica (context + cloned scene) each; a device may be
    listed more than once to rehearse the control flow on a one-GPU host (those replicas are gathered by device copies,
    distinct devices by ONE ncclGather inside the library)."""

    def __init__(self, flat_scene, devices, timing=False, options=None):
        self.ctxs, self.scenes = [], []
        for d in devices:
            ctx = Context(int(d), timing=timing)
            for k, v in (options or {}).items():
                ctx.set_option(k, v)
            self.ctxs.append(ctx)
            self.scenes.append(DeviceScene(flat_scene, ctx=ctx) if not self.scenes else self.scenes[0].clone(ctx))
        self._arr = (C.c_void_p * len(self.scenes))(*[s.handle for s in self.scenes])
        self.n = len(self.scenes)
        self._lit_frames = {}  # (nx, ny) -> the library's light-sampled frame object (rtmi_multi_lit_create), made on first use

    def set_option(self, name, value):
        for ctx in self.ctxs:
            ctx.set_option(name, value)

    def set_camera(self, camera):
        """DeviceScene.set_camera (the host form) on every replica -> True if any replica rebuilt its trees (they all do, or none)"""
        return any([s.set_camera(camera) for s in self.scenes])

    def set_materials(self, scene_or_flat):
        """DeviceScene.set_materials (the host form) on every replica -> True if the replicas rebuilt (they all do, or none).  The argument
        and fit checks of ALL replicas run before the first write: a bad edit raises and leaves every replica as it was."""
        f = scene_or_flat if isinstance(scene_or_flat, fl.FlatScene) else fl.flatten(scene_or_flat)
        for s in self.scenes:
            if len(f.prim_mat) != len(s.flat.prim_kind):
                raise ValueError("the edit has %d primitives, the scene %d" % (len(f.prim_mat), len(s.flat.prim_kind)))
        # the replicas are clones: they hold the same arrays, so the library's checks (creation's, on the scene's arrays with the edit in their
        # place) and its fit decision give one answer for all of them.  The host-only hook runs those checks without touching a scene.
        keep, args = core.scene_arrays(self.scenes[0].flat, **{name: getattr(f, name) for name in core.MATERIAL_FIELDS})
        h, facts = np.zeros(1, np.uint64), np.zeros(3, np.int32)
        check(_ffi.lib().rtmi_test_pack_materials(*args, 0, _ffi.ptr(h), _ffi.ptr(facts)))
        return any([s.set_materials(f) for s in self.scenes])

    def set_geometry(self, scene_or_flat, mode="auto"):
        """DeviceScene.set_geometry on every replica -> the first replica's info (the replicas are clones built from the same arrays: after the
        same sequence of edits they decide alike).  The structure checks of ALL replicas, and creation's checks of the edited arrays, run before
        the first replica is written: a bad edit raises and leaves every replica as it was."""
        if mode not in ("auto", "rebuild"):
            raise ValueError("mode must be 'auto' or 'rebuild'")
        pg, xp = [s._geometry_arrays(scene_or_flat) for s in self.scenes][0]
        keep, args = core.scene_arrays(self.scenes[0].flat, prim_geom=pg, xform_param=xp)
        h = np.zeros(1, np.uint64)
        check(_ffi.lib().rtmi_test_pack_geometry(*args, 0, _ffi.ptr(h)))
        return [s.set_geometry(scene_or_flat, mode) for s in self.scenes][0]

    def render(self, nx, ny, ns, depth=50, seed=0x5EED0002, precision="f64"):
        """host buffers: (linear [ny,nx,3] float64, rgb8, counters)"""
        lin, q, cnt = np.zeros((ny, nx, 3)), np.zeros((ny, nx, 3), np.uint8), np.zeros(2, np.uint64)
        check(_ffi.lib().rtmi_render_multi(self.n, self._arr, nx, ny, ns, depth, seed, {"f64": 0, "f32": 1}[precision],
                                           _ffi.ptr(lin), _ffi.ptr(q), _ffi.ptr(cnt)))
        return lin, q, cnt

    def render_device(self, nx, ny, ns, out_linear, out_rgb8, out_counters, depth=50, seed=0x5EED0002, precision="f64"):
        """outputs: device pointers / torch tensors on devices[0]; asynchronous on replica 0's context stream"""
        check(_ffi.lib().rtmi_render_multi_device(self.n, self._arr, nx, ny, ns, depth, seed, {"f64": 0, "f32": 1}[precision],
                                                  _ffi.ptr(out_linear), _ffi.ptr(out_rgb8), _ffi.ptr(out_counters)))

    # ---- one progressive / adaptive frame refined on all replicas (rtmi_render_multi_adaptive): DeviceScene's drivers, same defaults, same shapes ----
    def render_multi_adaptive(self, nx, ny, s_first, s_count, retire, eps=0.0, depth=core.DEFAULT_DEPTH, seed=core.RENDER_SEED, precision="f64"):
        """host buffers: samples [s_first, s_first + s_count) into the frame dealt over the replicas (retire: the adaptive rule with eps, else
        the progressive one) -> (linear, rgb8, stderr [ny,nx], samples int32 [ny,nx], counters)"""
        lin, q = np.zeros((ny, nx, 3)), np.zeros((ny, nx, 3), np.uint8)
        err, smp, cnt = np.zeros((ny, nx)), np.zeros((ny, nx), np.int32), np.zeros(2, np.uint64)
        check(_ffi.lib().rtmi_render_multi_adaptive(self.n, self._arr, nx, ny, s_first, s_count, int(retire), float(eps), depth, seed,
                                                    {"f64": 0, "f32": 1}[precision], _ffi.ptr(lin), _ffi.ptr(q), _ffi.ptr(err), _ffi.ptr(smp),
                                                    _ffi.ptr(cnt)))
        return lin, q, err, smp, cnt

    def render_progressive(self, nx, ny, s_first, s_count, depth=core.DEFAULT_DEPTH, seed=core.RENDER_SEED, precision="f64"):
        """DeviceScene.render_progressive for the whole frame, its tiles dealt over the replicas -> (linear, rgb8, stderr, counters), bit for bit
        the single context's"""
        lin, q, err, _, cnt = self.render_multi_adaptive(nx, ny, s_first, s_count, 0, 0.0, depth, seed, precision)
        return lin, q, err, cnt

    def refine(self, nx, ny, ns, chunk, depth=core.DEFAULT_DEPTH, seed=core.RENDER_SEED, precision="f64"):
        """DeviceScene.refine on all replicas: yields (k, linear, rgb8, stderr, counters) after every chunk"""
        if chunk <= 0 or ns <= 0:
            raise ValueError("ns and chunk must be > 0")
        k = 0
        while k < ns:
            n = min(chunk, ns - k)
            lin, q, err, cnt = self.render_progressive(nx, ny, k, n, depth, seed, precision)
            k += n
            yield k, lin, q, err, cnt

    def render_adaptive(self, nx, ny, s_first, s_count, eps, depth=core.DEFAULT_DEPTH, seed=core.RENDER_SEED, precision="f64"):
        """DeviceScene.render_adaptive for the whole frame, its tiles dealt over the replicas -> (linear, rgb8, stderr, samples, counters), bit
        for bit the single context's"""
        return self.render_multi_adaptive(nx, ny, s_first, s_count, 1, eps, depth, seed, precision)

    def render_adaptive_device(self, nx, ny, s_first, s_count, eps, out_linear=None, out_rgb8=None, out_stderr=None, out_samples=None,
                               out_counters=None, retire=True, depth=core.DEFAULT_DEPTH, seed=core.RENDER_SEED, precision="f64"):
        """the same with the outputs resident on devices[0] (rtmi_render_multi_adaptive_device; retire=False: the progressive rule); returns with
        every replica's stream synchronised"""
        check(_ffi.lib().rtmi_render_multi_adaptive_device(self.n, self._arr, nx, ny, s_first, s_count, int(bool(retire)), float(eps), depth, seed,
                                                           {"f64": 0, "f32": 1}[precision], _ffi.ptr(out_linear), _ffi.ptr(out_rgb8),
                                                           _ffi.ptr(out_stderr), _ffi.ptr(out_samples), _ffi.ptr(out_counters)))

    def adaptive_status(self):
        """(tiles still active, tiles of the frame, sum over the pixels of the samples their tile holds), summed over the replicas"""
        a, t, n = 0, 0, 0
        for ctx in self.ctxs:
            x, y, z = ctx.adaptive_status()
            a, t, n = a + x, t + y, n + z
        return a, t, n

    def adaptive_active_tiles(self):
        """global tile indices of the tiles still active on any replica, int32, ascending"""
        return np.sort(np.concatenate([ctx.adaptive_active_tiles() for ctx in self.ctxs])).astype(np.int32)

    def adaptive_retire(self, noise, eps):
        """Context.adaptive_retire with the whole-frame map on every replica (each reads its own active tiles) -> tiles retired in all"""
        return sum(ctx.adaptive_retire(noise, eps) for ctx in self.ctxs)

    def progressive_samples(self):
        """k of the frame (the replicas agree; 0 = none)"""
        ks = {ctx.progressive_samples() for ctx in self.ctxs}
        return ks.pop() if len(ks) == 1 else 0

    def progressive_release(self):
        for ctx in self.ctxs:
            ctx.progressive_release()

    def refine_adaptive(self, nx, ny, ns, chunk, eps, first=None, depth=core.DEFAULT_DEPTH, seed=core.RENDER_SEED, precision="f64"):
        """DeviceScene.refine_adaptive on all replicas: yields (k, linear, rgb8, stderr, samples, counters, active tiles) after every round and
        ends when no tile is active anywhere or k reaches ns"""
        first = chunk if first is None else first
        if chunk <= 0 or ns <= 0 or first <= 0:
            raise ValueError("ns, chunk and first must be > 0")
        k = 0
        while k < ns:
            n = min(first if k == 0 else chunk, ns - k)
            lin, q, err, smp, cnt = self.render_adaptive(nx, ny, k, n, eps, depth, seed, precision)
            k += n
            active = self.adaptive_status()[0]
            yield k, lin, q, err, smp, cnt, active
            if active == 0:
                break

    def refine_adaptive_denoised(self, nx, ny, ns, chunk, eps, first=None, na=core.FEATURE_SAMPLES, iterations=core.DENOISE_ITERATIONS,
                                 sigma_c=core.DENOISE_SIGMA_C, sigma_n=core.DENOISE_SIGMA_N, sigma_a=core.DENOISE_SIGMA_A,
                                 sigma_d=core.DENOISE_SIGMA_D, depth=core.DEFAULT_DEPTH, seed=core.RENDER_SEED, precision="f64"):
        """DeviceScene.refine_adaptive_denoised on all replicas: the features and the filter run on replica 0 over the assembled frame, the
        filtered noise map retires tiles on every replica.  Yields (k, linear, rgb8, stderr, samples, counters, active tiles after the
        retirement, filtered linear, filtered rgb8, filtered stderr) after every round."""
        first = chunk if first is None else first
        if chunk <= 0 or ns <= 0 or first <= 0:
            raise ValueError("ns, chunk and first must be > 0")
        ft, _ = self.scenes[0].render_features(nx, ny, na, seed, precision)
        k = 0
        while k < ns:
            n = min(first if k == 0 else chunk, ns - k)
            lin, q, err, smp, cnt = self.render_adaptive(nx, ny, k, n, 0.0, depth, seed, precision)
            k += n
            flt, fq, ferr = self.ctxs[0].denoise(lin, err, ft, iterations, sigma_c, sigma_n, sigma_a, sigma_d)
            self.adaptive_retire(ferr, eps)
            active = self.adaptive_status()[0]
            yield k, lin, q, err, smp, cnt, active, flt, fq, ferr
            if active == 0:
                break

    # ---- one light-sampled frame refined on all replicas (rtmi_multi_lit_*): DeviceScene's lit drivers, same defaults, same shapes ------------------
    def _lit_frame(self, nx, ny):
        """the library's frame object for nx x ny, created on first use and kept until close()"""
        key = (int(nx), int(ny))
        if key not in self._lit_frames:
            h = C.c_uint64(0)
            check(_ffi.lib().rtmi_multi_lit_create(self.n, self._arr, key[0], key[1], C.byref(h)))
            self._lit_frames[key] = h.value
        return self._lit_frames[key]

    def _lit_args(self, estimator, volume, lights, light_choice, depth, seed, precision):
        """-> the arguments of rtmi_multi_lit_render between s_count and the outputs, and what keeps the light list alive"""
        ds = self.scenes[0]
        if isinstance(estimator, str) and estimator == "ris":
            if volume:
                raise ValueError("estimator \"ris\" has no volume form")
            est = 3
        else:
            est = ds._tiles_estimator(estimator, volume)
        held, n_listed, _ = (None, 0, 0) if lights is None else ds._direct_lights(lights)
        return (int(depth), int(seed), est, n_listed, _ffi.ptr(held), ds._light_choice(light_choice), int(bool(volume))), held, {"f64": 0, "f32": 1}[precision]

    def lit_render(self, nx, ny, s_count, estimator="mis", volume=False, lights=None, light_choice=0, depth=core.DEFAULT_DEPTH, seed=core.RENDER_SEED,
                   precision="f64"):
        """rtmi_multi_lit_render: s_count more samples into every listed tile of the nx x ny frame -> (linear, rgb8, stderr [ny, nx], samples int32
        [ny, nx], the call's four counters summed over the replicas), host arrays, bit for bit one context's"""
        args, held, prec = self._lit_args(estimator, volume, lights, light_choice, depth, seed, precision)  # held: keeps the light list alive over the call
        lin, q = np.zeros((ny, nx, 3)), np.zeros((ny, nx, 3), np.uint8)
        err, smp, cnt = np.zeros((ny, nx)), np.zeros((ny, nx), np.int32), np.zeros(4, np.uint64)
        check(_ffi.lib().rtmi_multi_lit_render(self._lit_frame(nx, ny), prec, int(s_count), *args, _ffi.ptr(lin), _ffi.ptr(q), _ffi.ptr(err), _ffi.ptr(smp),
                                               _ffi.ptr(cnt)))
        return lin, q, err, smp, cnt

    def lit_render_device(self, nx, ny, s_count, out_linear=None, out_rgb8=None, out_stderr=None, out_samples=None, out_counters=None, estimator="mis",
                          volume=False, lights=None, light_choice=0, depth=core.DEFAULT_DEPTH, seed=core.RENDER_SEED, precision="f64"):
        """the same with the outputs resident on devices[0] (rtmi_multi_lit_render_device); returns with every replica's stream synchronised"""
        args, held, prec = self._lit_args(estimator, volume, lights, light_choice, depth, seed, precision)  # held: keeps the light list alive over the call
        check(_ffi.lib().rtmi_multi_lit_render_device(self._lit_frame(nx, ny), prec, int(s_count), *args, _ffi.ptr(out_linear), _ffi.ptr(out_rgb8),
                                                      _ffi.ptr(out_stderr), _ffi.ptr(out_samples), _ffi.ptr(out_counters)))

    def lit_retire(self, nx, ny, eps, noise=None):
        """rtmi_multi_lit_retire: every replica retires the tiles of its list whose pixels all pass noise <= eps (noise None: its own standard error;
        else a whole-frame [ny, nx] map -- a host array, or a torch tensor on devices[0]) -> tiles still listed on all replicas"""
        n = C.c_int32(0)
        if noise is None or isinstance(noise, np.ndarray):
            held = None if noise is None else np.ascontiguousarray(noise, np.float64)
            if held is not None and held.shape != (ny, nx):
                raise ValueError("noise must have shape (%d, %d)" % (ny, nx))
            check(_ffi.lib().rtmi_multi_lit_retire(self._lit_frame(nx, ny), _ffi.ptr(held), float(eps), C.byref(n)))
        else:
            check(_ffi.lib().rtmi_multi_lit_retire_device(self._lit_frame(nx, ny), _ffi.ptr(noise), float(eps), C.byref(n)))
        return n.value

    def lit_status(self, nx, ny):
        """(k = samples the frame's active tiles hold, tiles still listed on all replicas)"""
        k, a = C.c_int32(0), C.c_int32(0)
        check(_ffi.lib().rtmi_multi_lit_status(self._lit_frame(nx, ny), C.byref(k), C.byref(a)))
        return k.value, a.value

    def lit_active_tiles(self, nx, ny):
        """global tile indices still listed on any replica, int32, ascending"""
        out, n = np.zeros(max(1, n_tiles(nx, ny)), np.int32), C.c_int32(0)
        check(_ffi.lib().rtmi_multi_lit_active_tiles(self._lit_frame(nx, ny), len(out), _ffi.ptr(out), C.byref(n)))
        return out[:n.value].copy()

    def lit_reset(self, nx, ny):
        """k = 0 and every tile listed again (after a camera, material or geometry edit, or to start another frame)"""
        check(_ffi.lib().rtmi_multi_lit_reset(self._lit_frame(nx, ny)))

    def refine_lit(self, nx, ny, ns, chunk, estimator="mis", volume=False, lights=None, light_choice=0, depth=core.DEFAULT_DEPTH, seed=core.RENDER_SEED,
                   precision="f64"):
        """A fresh light-sampled frame refined uniformly on all replicas: yields (k, linear, rgb8, stderr, counters summed so far) after every chunk"""
        nx, ny, ns, chunk = int(nx), int(ny), int(ns), int(chunk)
        if nx <= 0 or ny <= 0 or ns <= 0 or chunk <= 0:
            raise ValueError("nx, ny, ns and chunk must be > 0")
        self.lit_reset(nx, ny)
        total, k = np.zeros(4, np.uint64), 0
        while k < ns:
            n = min(chunk, ns - k)
            lin, q, err, _, cnt = self.lit_render(nx, ny, n, estimator, volume, lights, light_choice, depth, seed, precision)
            total += cnt
            k += n
            yield k, lin, q, err, total.copy()

    def render_lit(self, nx, ny, ns, chunk=None, estimator="mis", volume=False, lights=None, light_choice=0, depth=core.DEFAULT_DEPTH,
                   seed=core.RENDER_SEED, precision="f64"):
        """DeviceScene.render_lit / render_lit_vol (volume=True) / render_lit_ris (estimator "ris") for the whole frame, its tiles dealt over the
        replicas -> (linear, rgb8, stderr, counters summed over the chunks), bit for bit the single context's"""
        out = None
        for out in self.refine_lit(nx, ny, ns, ns if chunk is None else chunk, estimator, volume, lights, light_choice, depth, seed, precision):
            pass
        return out[1:]

    def refine_lit_adaptive(self, nx, ny, ns, chunk, eps, first=None, estimator="mis", volume=False, lights=None, light_choice=0, denoised=False,
                            na=core.FEATURE_SAMPLES, iterations=core.DENOISE_ITERATIONS, sigma_c=core.DENOISE_SIGMA_C, sigma_n=core.DENOISE_SIGMA_N,
                            sigma_a=core.DENOISE_SIGMA_A, sigma_d=core.DENOISE_SIGMA_D, depth=core.DEFAULT_DEPTH, seed=core.RENDER_SEED, precision="f64"):
        """DeviceScene.refine_lit_adaptive on all replicas: every tile listed on its owner, then rounds of lit_render (`first` samples, default chunk,
        then `chunk`) each followed by lit_retire -- with denoised=True replica 0 renders the features once, filters the assembled frame each round
        and its filtered error is the map every replica retires by -- until no tile is listed or ns is reached.  -> (linear, rgb8, stderr, samples,
        counters summed over the rounds, rounds = [(k, tiles listed after the round's retirement, int32)]), bit for bit the single context's."""
        first = chunk if first is None else first
        if nx <= 0 or ny <= 0 or chunk <= 0 or ns <= 0 or first <= 0:
            raise ValueError("nx, ny, ns, chunk and first must be > 0")
        dn = (int(iterations), float(sigma_c), float(sigma_n), float(sigma_a), float(sigma_d))
        self.lit_reset(nx, ny)
        ft = self.scenes[0].render_features(nx, ny, na, seed, precision)[0] if denoised else None
        total, rounds, k, active = np.zeros(4, np.uint64), [], 0, n_tiles(nx, ny)
        lin = q = err = smp = None
        while k < ns and active:
            n = min(first if k == 0 else chunk, ns - k)
            lin, q, err, smp, cnt = self.lit_render(nx, ny, n, estimator, volume, lights, light_choice, depth, seed, precision)
            total += cnt
            k += n
            active = self.lit_retire(nx, ny, eps, self.ctxs[0].denoise(lin, err, ft, *dn)[2] if denoised else None)
            rounds.append((k, self.lit_active_tiles(nx, ny)))
        return lin, q, err, smp, total, rounds

    def sync(self):
        """wait for every replica (a multi render is complete when replica 0's stream is; the others finished before the gather)"""
        for ctx in self.ctxs:
            torch.cuda.synchronize(ctx.device)

    def last_gather_ms(self):
        ms = C.c_double()
        check(_ffi.lib().rtmi_last_gather_ms(self.ctxs[0].handle, C.byref(ms)))
        return ms.value

    def last_gather_path(self):
        """"none" | "same-device" | "peer-copy" | "rccl": how the last render moved the replicas' records to replica 0 (rtmi_last_gather_path)"""
        p = C.c_int32(-1)
        check(_ffi.lib().rtmi_last_gather_path(self.ctxs[0].handle, C.byref(p)))
        return _ffi.GATHER_PATHS[p.value]

    def last_trace_ms(self):
        """per replica: (sum of trace-kernel ms, launches) since the last call"""
        return [ctx.last_trace_ms() for ctx in self.ctxs]

    def close(self):
        for h in self._lit_frames.values():  # the frames go before their scenes
            _ffi.lib().rtmi_multi_lit_destroy(h)
        self._lit_frames = {}
        for s in self.scenes:
            s.close()
        for c in self.ctxs:
            c.close()
        self.scenes, self.ctxs = [], []


class FramePipeline:
    """`depth` frames in flight on one GPU: every slot owns a context (its own sample workspace and work queue), the scene
    and a stream, and consecutive frames go to consecutive slots.  A path tracer's launch ends with a die-off -- the last
    deep paths (up to `depth 50` bounces) finish in nearly empty waves; with two slots the next frame's workgroups take
    the CU slots the previous frame's workgroups vacate, and its gather / assemble overlap the next render as well.
    Frames are independent, so the images are those of the one-slot renderer (asserted in the GPU tests)."""

    def __init__(self, flat_scene, nx, ny, rank, world, device, depth=2, timing=False, options=None):
        self.slots = []
        for _ in range(max(1, depth)):
            ctx = Context(device, timing=timing)
            for k, v in (options or {}).items():
                ctx.set_option(k, v)
            ds = DeviceScene(flat_scene, ctx=ctx)
            self.slots.append((ctx, ds, TileRenderer(ds, nx, ny, rank, world), torch.cuda.Stream(device=device)))
        self.next = 0
        torch.cuda.synchronize(device)  # the slots' buffers were filled on the current stream

    def set_option(self, name, value):
        for ctx, _, _, _ in self.slots:
            ctx.set_option(name, value)

    def step(self, ns, camera=None, **kw):
        """enqueue one frame on the next slot; returns that slot's TileRenderer (its buffers are valid after sync()).  camera: the slot's own
        scene takes it in stream order before its frame (DeviceScene.set_camera's stream form: the host is not waited for, and the frames
        still in flight on the other slots keep their cameras -- every slot has a scene of its own)."""
        ctx, ds, tr, stream = self.slots[self.next]
        self.next = (self.next + 1) % len(self.slots)
        if tr.world == 1 and len(self.slots) > 1:
            if camera is not None:
                ds.set_camera(camera, stream=0)
            # one GPU, several frames in flight: every slot runs on its CONTEXT'S OWN stream (stream = NULL in the C-ABI).  The HIP
            # runtime deals streams to a few hardware queues in creation order; the contexts' streams are created back to back and
            # land on different queues, whereas extra torch streams were seen to share one queue (kernels of two frames then
            # run one after the other, no overlap).  No torch work is queued between frames, so nothing needs ordering with torch.
            tr._step(None, ns, kw.get("depth", 50), kw.get("seed", 0x5EED0002), kw.get("precision", "f64"))
            return tr
        with torch.cuda.stream(stream):
            if camera is not None:
                ds.set_camera(camera, stream=stream.cuda_stream)
            tr.step(ns, **kw)
        return tr

    def sync(self):
        for ctx, _, _, stream in self.slots:
            stream.synchronize()
        torch.cuda.synchronize(self.slots[0][0].device)  # the contexts' own streams

    def last_trace_ms(self):
        """(sum of trace-kernel durations in ms, number of launches) over all slots since the last call"""
        ms, n = 0.0, 0
        for ctx, _, _, _ in self.slots:
            a, b = ctx.last_trace_ms()
            ms, n = ms + a, n + b
        return ms, n

    def last_reduce_ms(self):
        """(sum of reduce_kernel durations in ms, launches) of the window the last last_trace_ms() closed"""
        ms, n = 0.0, 0
        for ctx, _, _, _ in self.slots:
            a, b = ctx.last_reduce_ms()
            ms, n = ms + a, n + b
        return ms, n

    def close(self):
        for ctx, ds, _, _ in self.slots:
            ds.close()
            ctx.close()
        self.slots = []
