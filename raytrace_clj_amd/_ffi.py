"""ctypes binding of librtmi.so (include/rtmi.h).  There is no CPU fallback: if the HIP library is
missing or no gfx950 device is visible, every entry point raises."""
import ctypes as C
import os

import numpy as np

# PyTorch-ROCm ships its own HIP runtime (torch/lib/libamdhip64.so, soname libamdhip64.so.7, + its own HSA runtime).
# Two HIP runtimes in one process cannot both own the GPU ("No HIP GPUs are available"), so when torch is the
# process's device-memory/stream/collective plumbing it must be loaded FIRST: librtmi.so's NEEDED libamdhip64.so.7
# then binds to the runtime that is already mapped.  (A torch-free host, e.g. the JVM via JNA, gets /opt/rocm's.)
try:
    import torch  # noqa: F401
except ImportError:  # pragma: no cover - torch-free host
    torch = None

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTMI_LIB") or os.path.join(_HERE, "lib", "librtmi.so")  # RTMI_LIB: experiment builds

# every symbol include/rtmi.h declares
SYMBOLS = [
    "rtmi_last_error", "rtmi_backend_name", "rtmi_version", "rtmi_init", "rtmi_shutdown", "rtmi_set_option",
    "rtmi_device_info", "rtmi_scene_create", "rtmi_scene_create_ex", "rtmi_scene_set_perlin", "rtmi_scene_set_images", "rtmi_scene_set_media_calls", "rtmi_scene_set_media_mode", "rtmi_scene_set_media_calls_narrowed", "rtmi_scene_device_bytes", "rtmi_scene_destroy", "rtmi_render", "rtmi_render_device",
    "rtmi_render_tiles_device", "rtmi_local_tiles", "rtmi_assemble_device", "rtmi_last_trace_ms", "rtmi_last_reduce_ms", "rtmi_probe_hit",
    "rtmi_probe_paths", "rtmi_probe_camera", "rtmi_probe_texture", "rtmi_probe_scatter", "rtmi_probe_rng",
    "rtmi_sample_key", "rtmi_test_half_outward", "rtmi_test_camera_fixed", "rtmi_test_build_tree", "rtmi_probe_arith", "rtmi_probe_math", "rtmi_probe_math2", "rtmi_last_traversal_counters",
    "rtmi_scene_clone", "rtmi_render_multi", "rtmi_render_multi_device", "rtmi_last_gather_ms",
    "rtmi_last_gather_path", "rtmi_rccl_probe", "rtmi_stream_idle", "rtmi_last_passes", "rtmi_last_record_reals", "rtmi_last_accel",
    "rtmi_render_progressive", "rtmi_render_progressive_device", "rtmi_progressive_samples", "rtmi_progressive_release",
    "rtmi_render_adaptive", "rtmi_render_adaptive_device", "rtmi_adaptive_status", "rtmi_adaptive_active_tiles",
    "rtmi_render_features", "rtmi_render_features_device", "rtmi_denoise", "rtmi_denoise_device",
    "rtmi_adaptive_retire", "rtmi_adaptive_retire_device",
    "rtmi_render_adaptive_tiles_device", "rtmi_assemble_progressive_device", "rtmi_render_multi_adaptive", "rtmi_render_multi_adaptive_device",
    "rtmi_scene_set_camera", "rtmi_scene_set_camera_stream", "rtmi_scene_camera",
    "rtmi_reproject", "rtmi_reproject_device",
    "rtmi_scene_tree_info",
    "rtmi_scene_set_materials", "rtmi_scene_set_materials_stream", "rtmi_test_pack_materials",
    "rtmi_scene_set_geometry", "rtmi_scene_last_refit_ms", "rtmi_test_pack_geometry", "rtmi_test_refit", "rtmi_test_refit_half", "rtmi_test_scene_nodes",
    "rtmi_render_rays", "rtmi_render_rays_device",
    "rtmi_test_stage_layout",
    "rtmi_query_hits", "rtmi_query_hits_device", "rtmi_query_occluded", "rtmi_query_occluded_device",
    "rtmi_occlusion_hemisphere", "rtmi_occlusion_hemisphere_device", "rtmi_occlusion_targets", "rtmi_occlusion_targets_device",
    "rtmi_ambient_occlusion", "rtmi_ambient_occlusion_device",
    "rtmi_scene_lights", "rtmi_test_scene_lights", "rtmi_direct_irradiance", "rtmi_direct_irradiance_device", "rtmi_render_direct", "rtmi_render_direct_device",
    "rtmi_render_rays_nee", "rtmi_render_rays_nee_device", "rtmi_probe_paths_nee",
    "rtmi_render_rays_mis", "rtmi_render_rays_mis_device", "rtmi_probe_paths_mis",
    "rtmi_render_lit", "rtmi_render_lit_device",
    "rtmi_render_rays_vol", "rtmi_render_rays_vol_device", "rtmi_probe_paths_vol", "rtmi_render_lit_vol", "rtmi_render_lit_vol_device",
    "rtmi_render_lit_tiles", "rtmi_render_lit_tiles_device", "rtmi_tiles_retire", "rtmi_tiles_retire_device",
    "rtmi_render_rays_ris", "rtmi_render_rays_ris_device", "rtmi_probe_paths_ris", "rtmi_render_lit_ris", "rtmi_render_lit_ris_device",
    "rtmi_lit_tiles_records_device", "rtmi_multi_lit_create", "rtmi_multi_lit_destroy", "rtmi_multi_lit_render", "rtmi_multi_lit_render_device",
    "rtmi_multi_lit_retire", "rtmi_multi_lit_retire_device", "rtmi_multi_lit_status", "rtmi_multi_lit_active_tiles", "rtmi_multi_lit_reset",
]

F64, F32 = 0, 1
ACCEL_FLAT, ACCEL_BVH = 0, 1
FLAG_TIMING = 1
GATHER_PATHS = {0: "none", 1: "same-device", 2: "peer-copy", 3: "rccl"}
SEG_REC = 12
TILE = 8
PROG_REC = 5  # doubles per pixel of a progressive tile record: mean rgb, stderr, samples
FEATURES = 8  # doubles per pixel of rtmi_render_features: albedo rgb, normal xyz, depth, coverage
HIT_REC = 12  # doubles per ray of rtmi_query_hits: hit?, prim, t, p xyz, normal xyz, u, v, material
RAYS_REC = 10  # doubles per group record of rtmi_render_rays: sums rgb, Welford mean rgb, Welford M2 rgb, count
DIRECT_REC = 4  # doubles per point record of rtmi_direct_irradiance / rtmi_render_direct: sum rgb, samples
NEE_REC = 24  # doubles per logged vertex of rtmi_probe_paths_nee: SEG_REC's twelve, state, light, d xyz, w, T rgb, contribution rgb
MIS_REC = 28  # doubles per logged vertex of rtmi_probe_paths_mis: NEE_REC's twenty-four, x, m, g, x' (closing vertex)
VOL_REC = 29  # doubles per logged vertex of rtmi_probe_paths_vol: MIS_REC's twenty-eight, then 1.0 at an Isotropic light-sampled vertex
RIS_REC = 32  # doubles per logged vertex of rtmi_probe_paths_ris: MIS_REC's twenty-eight for the chosen candidate, then S, w^ of the chosen one, r, live candidates
DIRECT_MAX_LIGHTS = 32  # RTMI_DIRECT_MAX_LIGHTS: lights one call samples
EDIT_STREAM_MAX_BYTES = 32768  # RTMI_EDIT_STREAM_MAX_BYTES: changed row payload one rtmi_scene_set_materials_stream call carries


class RtmiError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("rtmi error %d: %s" % (code, msg))
        self.code = code


_lib = None


def lib():
    """Load librtmi.so (built in-tree by `make -C raytrace_clj_amd/csrc` / __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RtmiError(-2, "HIP extension %s is missing; build it with `make -C raytrace_clj_amd/csrc` "
                            "(there is no CPU fallback)" % LIB_PATH)
    L = C.CDLL(LIB_PATH)
    vp, i32, i64, u64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double
    L.rtmi_last_error.restype = C.c_char_p
    L.rtmi_backend_name.restype = C.c_char_p
    L.rtmi_version.restype = C.c_int
    L.rtmi_init.argtypes = [C.c_int, C.c_uint32, C.POINTER(vp)]
    L.rtmi_shutdown.argtypes = [vp]
    L.rtmi_set_option.argtypes = [vp, C.c_char_p, i64]
    L.rtmi_device_info.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64), C.c_char_p, i32]
    L.rtmi_scene_create.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, C.POINTER(vp)]
    L.rtmi_scene_create_ex.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, C.POINTER(vp)]
    L.rtmi_scene_set_perlin.argtypes = [vp, vp, vp]
    L.rtmi_scene_set_images.argtypes = [vp, i32, vp, vp]
    L.rtmi_scene_set_media_calls.argtypes = [vp, i32, vp]
    L.rtmi_scene_set_media_mode.argtypes = [vp, i32]
    L.rtmi_scene_set_media_calls_narrowed.argtypes = [vp, i32, vp, vp]
    L.rtmi_scene_device_bytes.argtypes = [vp, C.POINTER(C.c_int64)]
    L.rtmi_scene_destroy.argtypes = [vp]
    L.rtmi_render.argtypes = [vp, i32, i32, i32, i32, u64, i32, i32, i32, i32, i32, vp, vp, vp]
    L.rtmi_render_device.argtypes = [vp, i32, i32, i32, i32, u64, i32, vp, vp, vp, vp]
    L.rtmi_render_tiles_device.argtypes = [vp, i32, i32, i32, i32, u64, i32, i32, i32, vp, vp, vp]
    L.rtmi_local_tiles.argtypes = [i32, i32, i32, i32]
    L.rtmi_local_tiles.restype = i32
    L.rtmi_assemble_device.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp]
    L.rtmi_last_trace_ms.argtypes = [vp, C.POINTER(dbl), C.POINTER(i32)]
    L.rtmi_last_reduce_ms.argtypes = [vp, C.POINTER(dbl), C.POINTER(i32)]
    L.rtmi_probe_hit.argtypes = [vp, i32, i32, vp, dbl, dbl, vp]
    L.rtmi_probe_paths.argtypes = [vp, i32, i32, vp, vp, u64, i32, vp, vp, vp, i32, vp]
    L.rtmi_probe_camera.argtypes = [vp, i32, i32, vp, vp, vp]
    L.rtmi_probe_texture.argtypes = [vp, i32, i32, i32, vp, vp]
    L.rtmi_probe_scatter.argtypes = [vp, i32, i32, i32, vp, vp, vp, vp]
    L.rtmi_probe_rng.argtypes = [vp, i32, u64, u64, i32, vp, vp]
    L.rtmi_sample_key.argtypes = [u64, u64, u64]
    L.rtmi_sample_key.restype = u64
    L.rtmi_probe_arith.argtypes = [vp, i32, vp, vp]
    L.rtmi_test_build_tree.argtypes = [i32, vp, vp, i32, vp, vp, vp]
    L.rtmi_test_half_outward.argtypes = [C.c_double, i32]
    L.rtmi_test_camera_fixed.argtypes = [i32, vp]
    L.rtmi_probe_math.argtypes = [vp, i32, vp, C.c_double, C.c_double, vp]
    L.rtmi_probe_math2.argtypes = [vp, i32, vp, C.c_double, C.c_double, i32, vp]
    L.rtmi_last_traversal_counters.argtypes = [vp, C.POINTER(u64), C.POINTER(u64)]
    L.rtmi_scene_clone.argtypes = [vp, vp, C.POINTER(vp)]
    L.rtmi_render_multi.argtypes = [i32, C.POINTER(vp), i32, i32, i32, i32, u64, i32, vp, vp, vp]
    L.rtmi_render_multi_device.argtypes = [i32, C.POINTER(vp), i32, i32, i32, i32, u64, i32, vp, vp, vp]
    L.rtmi_last_gather_ms.argtypes = [vp, C.POINTER(dbl)]
    L.rtmi_last_gather_path.argtypes = [vp, C.POINTER(i32)]
    L.rtmi_rccl_probe.argtypes = [C.c_char_p]
    L.rtmi_stream_idle.argtypes = [vp, C.POINTER(i32)]
    L.rtmi_last_passes.argtypes = [vp, C.POINTER(i32)]
    L.rtmi_last_record_reals.argtypes = [vp, C.POINTER(i32)]
    L.rtmi_last_accel.argtypes = [vp, C.POINTER(i32)]
    L.rtmi_render_progressive.argtypes = [vp, i32, i32, i32, i32, i32, u64, i32, i32, i32, i32, i32, vp, vp, vp, vp]
    L.rtmi_render_progressive_device.argtypes = [vp, i32, i32, i32, i32, i32, u64, i32, vp, vp, vp, vp, vp]
    L.rtmi_progressive_samples.argtypes = [vp, C.POINTER(i32)]
    L.rtmi_progressive_release.argtypes = [vp]
    L.rtmi_render_adaptive.argtypes = [vp, i32, i32, i32, i32, dbl, i32, u64, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.rtmi_render_adaptive_device.argtypes = [vp, i32, i32, i32, i32, dbl, i32, u64, i32, vp, vp, vp, vp, vp, vp]
    L.rtmi_adaptive_status.argtypes = [vp, C.POINTER(i32), C.POINTER(i32), C.POINTER(i64)]
    L.rtmi_adaptive_active_tiles.argtypes = [vp, i32, vp, C.POINTER(i32)]
    L.rtmi_adaptive_retire.argtypes = [vp, i32, i32, vp, dbl, C.POINTER(i32)]
    L.rtmi_adaptive_retire_device.argtypes = [vp, i32, i32, vp, dbl, C.POINTER(i32), vp]
    L.rtmi_render_features.argtypes =[vp, i32, i32, i32, u64, i32, i32, i32, i32, i32, vp, vp]
    L.rtmi_render_features_device.argtypes = [vp, i32, i32, i32, u64, i32, vp, vp, vp]
    L.rtmi_denoise.argtypes = [vp, i32, i32, vp, vp, vp, i32, dbl, dbl, dbl, dbl, vp, vp, vp]
    L.rtmi_denoise_device.argtypes = [vp, i32, i32, vp, vp, vp, i32, dbl, dbl, dbl, dbl, vp, vp, vp, vp]
    L.rtmi_render_adaptive_tiles_device.argtypes = [vp, i32, i32, i32, i32, i32, dbl, i32, u64, i32, i32, i32, vp, vp, vp]
    L.rtmi_assemble_progressive_device.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.rtmi_render_multi_adaptive.argtypes = [i32, C.POINTER(vp), i32, i32, i32, i32, i32, dbl, i32, u64, i32, vp, vp, vp, vp, vp]
    L.rtmi_render_multi_adaptive_device.argtypes = [i32, C.POINTER(vp), i32, i32, i32, i32, i32, dbl, i32, u64, i32, vp, vp, vp, vp, vp]
    L.rtmi_scene_set_camera.argtypes = [vp, i32, vp, C.POINTER(i32)]
    L.rtmi_scene_set_camera_stream.argtypes = [vp, i32, vp, vp]
    L.rtmi_scene_camera.argtypes = [vp, C.POINTER(i32), vp, C.POINTER(dbl), C.POINTER(dbl)]
    L.rtmi_scene_tree_info.argtypes = [vp, vp]
    L.rtmi_scene_set_materials.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, C.POINTER(i32)]
    L.rtmi_scene_set_materials_stream.argtypes = [vp, i32, vp, vp, vp, i32, vp, vp, vp, vp, vp]
    L.rtmi_test_pack_materials.argtypes = [i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, vp, vp]
    L.rtmi_scene_set_geometry.argtypes = [vp, i32, vp, i32, vp, i32, vp]
    L.rtmi_scene_last_refit_ms.argtypes = [vp, C.POINTER(dbl)]
    L.rtmi_test_pack_geometry.argtypes = [i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, vp, i32, vp, vp, i32, vp]
    L.rtmi_test_refit.argtypes = [i32, vp, vp, vp, i32, vp, i32, vp, i32, vp, vp, vp, i64, vp, vp, vp, vp, i64, vp]
    L.rtmi_test_refit_half.argtypes = [C.c_double, i32]
    L.rtmi_test_scene_nodes.argtypes = [vp, vp, i64, C.POINTER(i64)]
    L.rtmi_reproject.argtypes = [vp, i32, i32, i32, vp, i32, vp] + [vp] * 7 + [dbl] * 5 + [vp] * 5
    L.rtmi_reproject_device.argtypes = [vp, i32, i32, i32, vp, i32, vp] + [vp] * 7 + [dbl] * 5 + [vp] * 6
    L.rtmi_render_rays.argtypes = [vp, i32, i32, i32, i32, vp, vp, u64, C.c_uint32, i32, vp, vp, vp, vp, vp]
    L.rtmi_render_rays_device.argtypes = [vp, i32, i32, i32, i32, vp, vp, u64, C.c_uint32, i32, vp, vp, vp, vp, vp, vp]
    L.rtmi_test_stage_layout.argtypes = [i32, vp, vp, vp, vp, vp]
    L.rtmi_query_hits.argtypes = [vp, i32, i32, vp, vp, dbl, dbl, vp, C.c_uint32, vp, vp]
    L.rtmi_query_hits_device.argtypes = [vp, i32, i32, vp, vp, dbl, dbl, vp, C.c_uint32, vp, vp, vp]
    L.rtmi_query_occluded.argtypes = [vp, i32, i32, i32, vp, vp, dbl, dbl, vp, C.c_uint32, vp, vp, vp]
    L.rtmi_query_occluded_device.argtypes = [vp, i32, i32, i32, vp, vp, dbl, dbl, vp, C.c_uint32, vp, vp, vp, vp]
    L.rtmi_occlusion_hemisphere.argtypes = [vp, i32, i32, vp, vp, i32, i32, u64, dbl, dbl, dbl, vp, vp, vp, vp]
    L.rtmi_occlusion_hemisphere_device.argtypes = [vp, i32, i32, vp, vp, i32, i32, u64, dbl, dbl, dbl, vp, vp, vp, vp, vp]
    L.rtmi_occlusion_targets.argtypes = [vp, i32, i32, vp, vp, i32, vp, dbl, dbl, dbl, vp, vp, vp, vp]
    L.rtmi_occlusion_targets_device.argtypes = [vp, i32, i32, vp, vp, i32, vp, dbl, dbl, dbl, vp, vp, vp, vp, vp]
    L.rtmi_ambient_occlusion.argtypes = [vp, i32, i32, i32, i32, i32, dbl, u64, vp, vp, vp, vp]
    L.rtmi_ambient_occlusion_device.argtypes = [vp, i32, i32, i32, i32, i32, dbl, u64, vp, vp, vp, vp, vp]
    L.rtmi_scene_lights.argtypes = [vp, i32, vp, vp]
    L.rtmi_test_scene_lights.argtypes = [i32, vp, vp, vp, i32, vp, vp, i32, vp, vp, i32, vp, vp]
    L.rtmi_direct_irradiance.argtypes = [vp, i32, i32, vp, vp, i32, vp, i32, i32, u64, dbl, i32, vp, vp, vp, vp, vp, vp]
    L.rtmi_direct_irradiance_device.argtypes = [vp, i32, i32, vp, vp, i32, vp, i32, i32, u64, dbl, i32, vp, vp, vp, vp, vp, vp, vp]
    L.rtmi_render_direct.argtypes = [vp, i32, i32, i32, i32, i32, u64, vp, vp, vp, vp, vp]
    L.rtmi_render_direct_device.argtypes = [vp, i32, i32, i32, i32, i32, u64, vp, vp, vp, vp, vp, vp]
    L.rtmi_render_rays_nee.argtypes = [vp, i32, i32, i32, i32, vp, vp, u64, C.c_uint32, i32, i32, vp, vp, vp, vp, vp, vp]
    L.rtmi_render_rays_nee_device.argtypes = [vp, i32, i32, i32, i32, vp, vp, u64, C.c_uint32, i32, i32, vp, vp, vp, vp, vp, vp, vp]
    L.rtmi_probe_paths_nee.argtypes = [vp, i32, i32, vp, vp, u64, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    L.rtmi_render_rays_mis.argtypes = [vp, i32, i32, i32, i32, vp, vp, u64, C.c_uint32, i32, i32, vp, i32, vp, vp, vp, vp, vp]
    L.rtmi_render_rays_mis_device.argtypes = [vp, i32, i32, i32, i32, vp, vp, u64, C.c_uint32, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    L.rtmi_probe_paths_mis.argtypes = [vp, i32, i32, vp, vp, u64, i32, i32, vp, i32, vp, vp, vp, vp, i32, vp]
    L.rtmi_render_lit.argtypes = [vp, i32, i32, i32, i32, i32, i32, u64, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp]
    L.rtmi_render_lit_device.argtypes = [vp, i32, i32, i32, i32, i32, i32, u64, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rtmi_render_rays_vol.argtypes = [vp, i32, i32, i32, i32, vp, vp, u64, C.c_uint32, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp]
    L.rtmi_render_rays_vol_device.argtypes = [vp, i32, i32, i32, i32, vp, vp, u64, C.c_uint32, i32, i32, i32, vp, i32, vp, vp, vp, vp, vp, vp]
    L.rtmi_probe_paths_vol.argtypes = [vp, i32, i32, vp, vp, u64, i32, i32, i32, vp, i32, vp, vp, vp, vp, i32, vp]
    L.rtmi_render_lit_vol.argtypes = L.rtmi_render_lit.argtypes
    L.rtmi_render_lit_vol_device.argtypes = L.rtmi_render_lit_device.argtypes
    L.rtmi_render_lit_tiles.argtypes = [vp, i32, i32, i32, i32, i32, i32, u64, i32, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rtmi_render_lit_tiles_device.argtypes = [vp, i32, i32, i32, i32, i32, i32, u64, i32, i32, vp, i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rtmi_render_rays_ris.argtypes = L.rtmi_render_rays_nee.argtypes
    L.rtmi_render_rays_ris_device.argtypes = L.rtmi_render_rays_nee_device.argtypes
    L.rtmi_probe_paths_ris.argtypes = [vp, i32, i32, vp, vp, u64, i32, i32, vp, vp, vp, vp, vp, i32, vp]
    L.rtmi_render_lit_ris.argtypes = [vp, i32, i32, i32, i32, i32, i32, u64, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rtmi_render_lit_ris_device.argtypes = [vp, i32, i32, i32, i32, i32, i32, u64, i32, vp, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp]
    L.rtmi_tiles_retire.argtypes = [vp, i32, i32, vp, dbl, i32, vp, vp, C.POINTER(i32)]
    L.rtmi_tiles_retire_device.argtypes = [vp, i32, i32, vp, dbl, i32, vp, vp, C.POINTER(i32), vp]
    L.rtmi_lit_tiles_records_device.argtypes = [vp, i32, i32, i32, i32, i32, vp, vp, vp, vp, vp]
    L.rtmi_multi_lit_create.argtypes = [i32, C.POINTER(vp), i32, i32, C.POINTER(u64)]
    L.rtmi_multi_lit_destroy.argtypes = [u64]
    L.rtmi_multi_lit_render.argtypes = [u64, i32, i32, i32, u64, i32, i32, vp, i32, i32, vp, vp, vp, vp, vp]
    L.rtmi_multi_lit_render_device.argtypes = L.rtmi_multi_lit_render.argtypes
    L.rtmi_multi_lit_retire.argtypes = [u64, vp, dbl, C.POINTER(i32)]
    L.rtmi_multi_lit_retire_device.argtypes = L.rtmi_multi_lit_retire.argtypes
    L.rtmi_multi_lit_status.argtypes = [u64, C.POINTER(i32), C.POINTER(i32)]
    L.rtmi_multi_lit_active_tiles.argtypes = [u64, i32, vp, C.POINTER(i32)]
    L.rtmi_multi_lit_reset.argtypes = [u64]
    for name in SYMBOLS:
        fn = getattr(L, name)
        if fn.restype is C.c_int and name not in ("rtmi_version",):
            fn.restype = C.c_int
    _lib = L
    return L


def check(rc):
    if rc != 0:
        raise RtmiError(rc, lib().rtmi_last_error().decode("utf-8", "replace"))


def ptr(a):
    """device or host pointer of a numpy array / torch tensor / int / None"""
    if a is None:
        return None
    if isinstance(a, int):
        return C.c_void_p(a)
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(C.c_void_p)
    if hasattr(a, "data_ptr"):
        return C.c_void_p(a.data_ptr())
    raise TypeError("cannot take a pointer of %r" % type(a))
