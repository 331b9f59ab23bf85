"""ctypes view of include/rtx_hip.h (the C ABI of librtx_hip.so).

The library is the product: if it is missing or cannot be loaded this module raises --
there is no Python/NumPy/CPU fallback for the render path.
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("RTX_HIP_LIB") or os.path.join(HERE, "librtx_hip.so")   # RTX_HIP_LIB: A/B builds
# the lab library: same sources with -DRTX_LAB, same ABI, same dispatch, + the rtx_debug_* hooks and the A/B forms behind the
# RTX_TUNE_LAB_MASK bits (include/rtx_hip.h, "Product and lab").  Loaded only for a Config that asks for it (Config.lab / a lab tuning bit).
LAB_LIB_PATH = os.environ.get("RTX_HIP_LAB_LIB") or os.path.join(HERE, "librtx_hip_lab.so")

RTX_SPHERE, RTX_PLANE, RTX_TRIANGLE = 0, 1, 2
RTX_KERNEL_AUTO, RTX_KERNEL_EXACT, RTX_KERNEL_MIXED, RTX_KERNEL_MIXED_VERIFY, RTX_KERNEL_BVH, RTX_KERNEL_BVH_REGROUP = 0, 1, 2, 3, 4, 5
RTX_KERNEL_WAVEFRONT = 6
# RtxConfig.tuning bits (include/rtx_hip.h): A/B switches, every combination renders the same bits
# (bits 1, 19, 21, 22, 24 and 26 are retired: refused by both libraries, never to be reused)
RTX_TUNE_NO_TILES, RTX_TUNE_NO_QNODES, RTX_TUNE_NO_PACKETS = 1, 4, 8
RTX_TUNE_WF_PURE, RTX_TUNE_ONE_STAGE, RTX_TUNE_TWO_STAGE, RTX_TUNE_BVH_MEDIAN = 16, 32, 64, 128
RTX_TUNE_TRI_LEAF_SHIFT, RTX_TUNE_THRESH_SHIFT = 8, 12
RTX_TUNE_PK_LDS_STACK = 1 << 20
RTX_TUNE_NO_CUT = 1 << 23
RTX_TUNE_HALVES = 1 << 27
RTX_TUNE_NO_HALVES = 1 << 28
RTX_TUNE_NO_TILE_LISTS = 1 << 29
RTX_TUNE_INLINE_LEAVES = 1 << 25
RTX_TUNE_LAB_MASK = RTX_TUNE_NO_QNODES | RTX_TUNE_NO_PACKETS | RTX_TUNE_WF_PURE | RTX_TUNE_PK_LDS_STACK | RTX_TUNE_INLINE_LEAVES
RTX_TUNE_KNOWN_MASK = (RTX_TUNE_LAB_MASK | RTX_TUNE_NO_TILES | RTX_TUNE_ONE_STAGE | RTX_TUNE_TWO_STAGE | RTX_TUNE_BVH_MEDIAN |
                       (15 << RTX_TUNE_TRI_LEAF_SHIFT) | (127 << RTX_TUNE_THRESH_SHIFT) | RTX_TUNE_NO_CUT | RTX_TUNE_HALVES | RTX_TUNE_NO_HALVES | RTX_TUNE_NO_TILE_LISTS)
RTX_UPDATE_AUTO, RTX_UPDATE_REBUILD, RTX_UPDATE_DEFORM = 0, 1, 2
RTX_UPDATED_NOTHING, RTX_UPDATED_RECORDS, RTX_UPDATED_REFIT, RTX_UPDATED_REBUILT = 0, 1, 2, 3
RTX_MULTI_HIT_MAX = 32                       # rtx_scene_multi_hits: 1 <= k <= this
RTX_DENOISE_MAX_PASSES, RTX_DENOISE_DEMODULATE, RTX_DENOISE_NO_NORMAL = 8, 1, 0xFFFFFFFF   # RtxDenoiseParams
RTX_UPSAMPLE_MAX_FACTOR, RTX_UPSAMPLE_DEMODULATE = 8, 1                                     # RtxUpsampleParams
RTX_OK, RTX_ERR_INVALID_ARGUMENT, RTX_ERR_NO_DEVICE, RTX_ERR_HIP, RTX_ERR_UNSUPPORTED, RTX_ERR_OUT_OF_MEMORY = range(6)

# RtxObject, 136 bytes: one entry of Scene.objects (scene.rs:80; object.rs:9-15,78-86)
OBJECT_DTYPE = np.dtype([
    ("kind", "<u4"), ("reserved", "<u4"), ("geom", "<f8", (9,)),
    ("base_color", "<f8", (3,)), ("emission_color", "<f8", (3,)), ("roughness", "<f8"),
])
assert OBJECT_DTYPE.itemsize == 136


class RtxConfig(C.Structure):
    _fields_ = [("rays_per_pixel", C.c_uint64), ("max_bounces", C.c_uint64),
                ("focal_length", C.c_double), ("focal_offset", C.c_double), ("non_focal_offset", C.c_double),
                ("seed", C.c_uint64), ("kernel", C.c_uint32), ("tuning", C.c_uint32)]


class RtxCamera(C.Structure):
    _fields_ = [("fov", C.c_double), ("position", C.c_double * 3), ("direction", C.c_double * 3),
                ("to_cam_space", C.c_double * 9), ("to_world_space", C.c_double * 9)]


class RtxScene(C.Structure):
    _fields_ = [("config", RtxConfig), ("camera", RtxCamera), ("n_objects", C.c_uint64), ("objects", C.c_void_p)]


class RtxStats(C.Structure):
    _fields_ = [("primary_rays", C.c_uint64), ("segments", C.c_uint64), ("exact_tests", C.c_uint64),
                ("filter_tests", C.c_uint64), ("trace_ms", C.c_double), ("resolve_ms", C.c_double),
                ("filter_mismatches", C.c_uint64), ("box_tests", C.c_uint64),
                ("trace_launches", C.c_uint32), ("kernel", C.c_uint32),
                ("stage1_ms", C.c_double), ("stage1_box_tests", C.c_uint64), ("stage1_filter_tests", C.c_uint64),
                ("stage1_exact_tests", C.c_uint64)]


class RtxRay(C.Structure):
    _fields_ = [("position", C.c_double * 3), ("direction", C.c_double * 3)]


class RtxHit(C.Structure):
    _fields_ = [("position", C.c_double * 3), ("normal", C.c_double * 3), ("distance", C.c_double), ("object", C.c_int64)]


class RtxPixelFeatures(C.Structure):
    _fields_ = [("albedo", C.c_double * 3), ("emission", C.c_double * 3), ("normal", C.c_double * 3), ("depth", C.c_double),
                ("coverage", C.c_double), ("object", C.c_int64)]


class RtxDenoiseParams(C.Structure):
    _fields_ = [("passes", C.c_uint32), ("flags", C.c_uint32), ("normal_power_log2", C.c_uint32), ("reserved", C.c_uint32),
                ("sigma_color", C.c_double), ("sigma_depth", C.c_double), ("sigma_albedo", C.c_double), ("epsilon", C.c_double),
                ("albedo_min", C.c_double)]


class RtxUpsampleParams(C.Structure):
    _fields_ = [("factor", C.c_uint32), ("flags", C.c_uint32), ("normal_power_log2", C.c_uint32), ("reserved", C.c_uint32),
                ("sigma_depth", C.c_double), ("sigma_albedo", C.c_double), ("albedo_min", C.c_double), ("min_weight", C.c_double)]


class RtxTemporalParams(C.Structure):
    _fields_ = [("alpha_min", C.c_double), ("max_history", C.c_double), ("plane_tolerance", C.c_double), ("normal_min", C.c_double),
                ("min_weight", C.c_double), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


RTX_MOTION_LOST = 0xFFFFFFFF                    # RtxObjectMotion.kind: no previous geometry to rewind to


class RtxObjectMotion(C.Structure):
    _fields_ = [("kind", C.c_uint32), ("reserved", C.c_uint32), ("now", C.c_double * 9), ("before", C.c_double * 9)]


# the same layouts as numpy records (arrays of rays / answers)
RAY_DTYPE = np.dtype([("position", "<f8", (3,)), ("direction", "<f8", (3,))])
HIT_DTYPE = np.dtype([("position", "<f8", (3,)), ("normal", "<f8", (3,)), ("distance", "<f8"), ("object", "<i8")])
FEATURE_DTYPE = np.dtype([("albedo", "<f8", (3,)), ("emission", "<f8", (3,)), ("normal", "<f8", (3,)), ("depth", "<f8"),
                          ("coverage", "<f8"), ("object", "<i8")])
assert RAY_DTYPE.itemsize == C.sizeof(RtxRay) == 48 and HIT_DTYPE.itemsize == C.sizeof(RtxHit) == 64
assert FEATURE_DTYPE.itemsize == C.sizeof(RtxPixelFeatures) == 96
DENOISE_PARAMS_DTYPE = np.dtype([("passes", "<u4"), ("flags", "<u4"), ("normal_power_log2", "<u4"), ("reserved", "<u4"),
                                 ("sigma_color", "<f8"), ("sigma_depth", "<f8"), ("sigma_albedo", "<f8"), ("epsilon", "<f8"),
                                 ("albedo_min", "<f8")])
assert DENOISE_PARAMS_DTYPE.itemsize == C.sizeof(RtxDenoiseParams) == 56
TEMPORAL_PARAMS_DTYPE = np.dtype([("alpha_min", "<f8"), ("max_history", "<f8"), ("plane_tolerance", "<f8"), ("normal_min", "<f8"),
                                  ("min_weight", "<f8"), ("flags", "<u4"), ("reserved", "<u4")])
assert TEMPORAL_PARAMS_DTYPE.itemsize == C.sizeof(RtxTemporalParams) == 48
UPSAMPLE_PARAMS_DTYPE = np.dtype([("factor", "<u4"), ("flags", "<u4"), ("normal_power_log2", "<u4"), ("reserved", "<u4"),
                                  ("sigma_depth", "<f8"), ("sigma_albedo", "<f8"), ("albedo_min", "<f8"), ("min_weight", "<f8")])
assert UPSAMPLE_PARAMS_DTYPE.itemsize == C.sizeof(RtxUpsampleParams) == 48
OBJECT_MOTION_DTYPE = np.dtype([("kind", "<u4"), ("reserved", "<u4"), ("now", "<f8", (9,)), ("before", "<f8", (9,))])
assert OBJECT_MOTION_DTYPE.itemsize == C.sizeof(RtxObjectMotion) == 152


# every symbol include/rtx_hip.h declares: (name, restype, argtypes)
SYMBOLS = [
    ("rtx_version", C.c_int32, []),
    ("rtx_last_error", C.c_char_p, []),
    ("rtx_device_count", C.c_int32, []),
    ("rtx_lab_build", C.c_int32, []),
    ("rtx_camera_new", C.c_int32, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_double, C.POINTER(RtxCamera)]),
    ("rtx_render", C.c_int32, [C.POINTER(RtxScene), C.c_uint32, C.c_uint32, C.c_void_p]),
    ("rtx_render_to_image", C.c_int32, [C.POINTER(RtxScene), C.c_uint32, C.c_uint32, C.c_void_p]),
    ("rtx_render_devices", C.c_int32, [C.POINTER(RtxScene), C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.c_uint32, C.c_void_p]),
    ("rtx_render_to_image_devices", C.c_int32, [C.POINTER(RtxScene), C.c_uint32, C.c_uint32, C.POINTER(C.c_int32), C.c_uint32,
                                                C.c_void_p]),
    ("rtx_scene_upload", C.c_int32, [C.POINTER(RtxScene), C.c_int32, C.POINTER(C.c_void_p)]),
    ("rtx_scene_free", C.c_int32, [C.c_void_p]),
    ("rtx_scene_set_config", C.c_int32, [C.c_void_p, C.POINTER(RtxConfig)]),
    ("rtx_scene_set_scratch_limit", C.c_int32, [C.c_void_p, C.c_uint64]),
    ("rtx_scene_set_camera", C.c_int32, [C.c_void_p, C.POINTER(RtxCamera)]),
    ("rtx_scene_append_objects", C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64]),
    ("rtx_scene_update_objects", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]),
    ("rtx_scene_set_visible", C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.POINTER(C.c_uint32)]),
    ("rtx_scene_get_visible", C.c_int32, [C.c_void_p, C.c_void_p]),
    ("rtx_render_rows", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                    C.c_void_p, C.c_void_p, C.POINTER(RtxStats)]),
    ("rtx_blocks_row_count", C.c_uint32, [C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32]),
    ("rtx_render_blocks", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                      C.c_void_p, C.c_void_p, C.POINTER(RtxStats)]),
    ("rtx_render_blocks_accumulate", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64,
                                                 C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtxStats)]),
    ("rtx_scene_closest_hits", C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(RtxStats)]),
    ("rtx_scene_primary_hits", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(RtxStats)]),
    ("rtx_closest_hits", C.c_int32, [C.POINTER(RtxScene), C.c_void_p, C.c_uint64, C.c_void_p]),
    ("rtx_scene_any_hits", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.POINTER(RtxStats)]),
    ("rtx_any_hits", C.c_int32, [C.POINTER(RtxScene), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    ("rtx_scene_multi_hits", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.POINTER(RtxStats)]),
    ("rtx_scene_primary_multi_hits", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.POINTER(RtxStats)]),
    ("rtx_multi_hits", C.c_int32, [C.POINTER(RtxScene), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("rtx_scene_trace_paths", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(RtxStats)]),
    ("rtx_trace_paths", C.c_int32, [C.POINTER(RtxScene), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("rtx_scene_trace_samples", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.POINTER(RtxStats)]),
    ("rtx_render_blocks_refine", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_uint32,
                                             C.c_uint32, C.c_uint32, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p,
                                             C.POINTER(C.c_uint64), C.c_void_p, C.POINTER(RtxStats)]),
    ("rtx_trace_samples", C.c_int32, [C.POINTER(RtxScene), C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
    ("rtx_scene_pixel_features", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.POINTER(RtxStats)]),
    ("rtx_scene_pixel_features_blocks", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                                    C.c_void_p, C.c_void_p, C.POINTER(RtxStats)]),
    ("rtx_pixel_features", C.c_int32, [C.POINTER(RtxScene), C.c_uint32, C.c_uint32, C.c_void_p]),
    ("rtx_quantize_image_device", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_int32, C.c_void_p]),
    ("rtx_denoise_default_params", None, [C.c_void_p]),
    ("rtx_denoise_work_bytes", C.c_uint64, [C.c_uint32, C.c_uint32, C.c_void_p]),
    ("rtx_denoise_device", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_int32, C.c_void_p]),
    ("rtx_denoise", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rtx_temporal_default_params", None, [C.c_void_p]),
    ("rtx_temporal_tables", C.c_int32, [C.c_double, C.c_uint32, C.c_uint32, C.c_void_p]),
    ("rtx_temporal_accumulate_device", C.c_int32, [C.c_void_p] * 9 + [C.c_uint32, C.c_uint32] + [C.c_void_p] * 5 + [C.c_int32, C.c_void_p]),
    ("rtx_temporal_accumulate", C.c_int32, [C.c_void_p] * 8 + [C.c_uint32, C.c_uint32] + [C.c_void_p] * 5),
    ("rtx_rewind_hits_device", C.c_int32, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_int32,
                                           C.c_void_p]),
    ("rtx_rewind_hits", C.c_int32, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]),
    ("rtx_object_motions", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rtx_upsample_default_params", None, [C.c_void_p]),
    ("rtx_upsample_device", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_void_p]),
    ("rtx_upsample", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]),
    ("rtx_debug_math", C.c_int32, [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    ("rtx_debug_paths", C.c_int32, [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]),
    ("rtx_debug_store_samples", C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]),
    ("rtx_debug_resolve", C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint64, C.c_int32,
                                      C.c_int32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64]),
    ("rtx_debug_path_bounds", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_uint32]),
    ("rtx_debug_resolve_moments", C.c_int32, [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint64,
                                              C.c_void_p, C.c_uint64]),
    ("rtx_debug_gather", C.c_int32, [C.c_int32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32,
                                     C.c_void_p]),
    ("rtx_debug_host_scene", C.c_int32, [C.POINTER(RtxScene), C.POINTER(C.c_uint64)]),
    ("rtx_debug_host_refit", C.c_int32, [C.POINTER(RtxScene), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64),
                                         C.POINTER(C.c_uint32), C.POINTER(C.c_uint64)]),
    ("rtx_debug_resident_digests", C.c_int32, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("rtx_debug_host_refit_mesh", C.c_int32, [C.POINTER(RtxScene), C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64),
                                              C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_double)]),
    ("rtx_debug_resident_mesh_digests", C.c_int32, [C.c_void_p, C.POINTER(C.c_uint64)]),
    ("rtx_debug_host_set_visible", C.c_int32, [C.POINTER(RtxScene), C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.POINTER(C.c_double), C.c_void_p, C.c_void_p,
                                               C.c_uint64]),
    ("rtx_debug_tile_lists", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]),
    ("rtx_debug_sweep_filter", C.c_int32, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]),
]


class RtxError(RuntimeError):
    def __init__(self, status, message):
        super().__init__("librtx_hip status %d: %s" % (status, message))
        self.status = status


_libs = {}


def _share_hip_runtime_with_torch():
    """One HIP runtime per process.  PyTorch-ROCm wheels bundle their own libamdhip64.so (SONAME
    libamdhip64.so.7, the same SONAME as /opt/rocm's).  If it is mapped before librtx_hip.so, the dynamic
    linker resolves our NEEDED libamdhip64.so.7 to it, and torch tensors' device pointers, streams and our
    launches all live in one runtime.  torch itself is not imported here."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass


def load_library(lab=False):
    """dlopen librtx_hip.so (lab=True: librtx_hip_lab.so) and bind every entry point.  Raises if the library is absent."""
    lab = bool(lab)
    if lab in _libs:
        return _libs[lab]
    path = LAB_LIB_PATH if lab else LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(
            "%s is not built (%s). Build it with `python rust-raytracing_amd/build.py` "
            "(hipcc, gfx950). There is no CPU fallback for the render path." % (os.path.basename(path), path))
    _share_hip_runtime_with_torch()
    lib = C.CDLL(path)                   # RTLD_LOCAL: the two libraries export the same names and stay apart
    for name, restype, argtypes in SYMBOLS:
        fn = getattr(lib, name)          # AttributeError if the symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    if "RTX_HIP_LIB" not in os.environ and "RTX_HIP_LAB_LIB" not in os.environ and int(lib.rtx_lab_build()) != int(lab):
        raise RuntimeError("%s reports rtx_lab_build() = %d" % (path, int(lib.rtx_lab_build())))
    _libs[lab] = lib
    return lib


def check(status, lib=None):
    if status != 0:
        msg = (lib or load_library()).rtx_last_error()
        raise RtxError(status, msg.decode("utf-8", "replace") if msg else "")
